"""Jump-forward for the regex guide without a GPU: the definition (tests/jump_ref.py) pinned by hand with compiled patterns, and the
code the kernels run (splintr_amd/csrc/spl_k_dfa_jump.h, evaluated by tests/hostsim/jump_sim.cpp with 64, 5, 3 and 1 lanes) against that
definition through the checks of tests/jump_cases.py -- force, runs and their lengths, the jump step over poisoned outputs with every
store counted, adversarial jump tables, KEEP_FREE, layouts, the all-zero index against the plain step's simulation -- plus two mutants
of the header that a named check must catch, and the C ABI's refusals through the real library."""
import ctypes

import numpy as np
import pytest

import dfa_ref as ref
import jump_cases as cases
import jump_ref as jref

LANES = [64, 5, 3, 1]
NAMES = sorted(cases.TOYS)
SPL_EINVAL = -1
JSON = r'\{"name": "[a-z]+", "age": [0-9]{1,3}\}'
TOOL = r"<tool>(get_weather|get_time)</tool>"


@pytest.fixture(scope="module")
def sim():
    import jump_sim
    jump_sim.lib()
    return jump_sim


def runners(sim, name, lanes=64, mutant=""):
    import dfa_sim
    vocab, specials = cases.TOYS[name]()
    v = sim.Vocab(vocab, specials)

    def run(table, n_states, **kw):
        return sim.run(v, table, n_states, lanes=lanes, mutant=mutant, **kw)

    def runs(table, n_states):
        return sim.runs(table, n_states, lanes=lanes, mutant=mutant)

    def step(table, n_states, **kw):
        return dfa_sim.run(v, table, n_states, lanes=lanes, **kw)
    return run, runs, step


# ---------------------------------------------------------------------------------------------- the definition, by hand
def _state_behind(tab, data):
    q = ref.walk(tab, 0, data)
    assert q != ref.DEAD
    return q


def test_ref_json_object():
    tab = cases.compiled(JSON)
    assert ref.n_states(tab) == 26
    assert jref.run(tab, 0) == b'{"name": "'
    assert jref.run(tab, _state_behind(tab, b'{"name": "bob"')) == b', "age": '
    inside_name = _state_behind(tab, b'{"name": "bo')
    assert jref.run(tab, inside_name) == b"" and jref.force(tab, inside_name) is None
    assert jref.run(tab, _state_behind(tab, b'{"name": "b')) == b""
    head = b'{"name": "bob", "age": '
    assert jref.run(tab, _state_behind(tab, head)) == b""                      # a digit: ten bytes to choose from
    assert jref.run(tab, _state_behind(tab, head + b"4")) == b""               # a digit or }
    assert jref.run(tab, _state_behind(tab, head + b"42")) == b""
    assert jref.run(tab, _state_behind(tab, head + b"421")) == b"}"            # } is forced only behind the third digit
    assert jref.run(tab, _state_behind(tab, head + b"421}")) == b""            # accepts: never forced
    assert sum(1 for q in range(26) if jref.force(tab, q) is not None) == sum(len(r) for r in (b'{"name": "', b', "age": ', b"}"))


def test_ref_tool_call():
    tab = cases.compiled(TOOL)
    assert ref.n_states(tab) == 28
    assert jref.run(tab, 0) == b"<tool>get_"
    assert jref.run(tab, _state_behind(tab, b"<tool>get_w")) == b"eather</tool>"
    assert jref.run(tab, _state_behind(tab, b"<tool>get_t")) == b"ime</tool>"
    assert jref.run(tab, _state_behind(tab, b"<tool>get_")) == b""


def _yes_table():
    """yes|no|yellow by hand: 0 -y-> 1 -e-> 2 -s-> 3* ; 2 -l-> 4 -l-> 5 -o-> 6 -w-> 3* ; 0 -n-> 7 -o-> 3*   (3 accepts)"""
    t = np.full((8, 256), ref.DEAD, dtype=np.uint16)
    for q, x, to in ((0, "y", 1), (1, "e", 2), (2, "s", 3), (2, "l", 4), (4, "l", 5), (5, "o", 6), (6, "w", 3), (0, "n", 7), (7, "o", 3)):
        t[q, ord(x)] = to
    return t, np.array([0, 0, 0, 1, 0, 0, 0, 0], dtype=np.uint8)


def test_ref_yes_no_yellow_by_hand():
    tab = _yes_table()
    assert jref.runs(tab) == [b"", b"e", b"", b"", b"low", b"ow", b"w", b"o"]
    assert [jref.force(tab, q) for q in range(8)] == [None, ord("e"), None, None, ord("l"), ord("o"), ord("w"), ord("o")]
    arr, lens = jref.run_arrays(tab)
    assert lens.tolist() == [0, 1, 0, 0, 3, 2, 1, 1] and bytes(arr[4]) == b"low" + bytes(61)
    # a transition value >= S counts as dead: 8 and 0x1234 beside the one live byte change nothing; with a ninth state the 8s are alive
    t2 = tab[0].copy()
    t2[7, ord("x")], t2[7, ord("z")], t2[1, 0] = 8, 0x1234, 8
    assert jref.runs((t2, tab[1])) == jref.runs(tab)
    t3 = np.concatenate([t2, np.full((1, 256), ref.DEAD, dtype=np.uint16)])
    assert jref.force((t3, np.append(tab[1], 0)), 7) is None and jref.force((t3, np.append(tab[1], 0)), 1) is None
    # the jump by the definition: "yel" arrives at 4, whose row spells "low" as one id; a row that does not walk emits nothing
    toks = ref.ordinary({0: b"y", 1: b"ye", 2: b"yes", 3: b"yel", 4: b"n", 5: b"no", 6: b"low", 7: b"o", 8: b"w"})
    ids = np.zeros((8, 64), dtype=np.uint32)
    n = np.zeros(8, dtype=np.uint8)
    ids[4, 0], n[4] = 6, 1
    ids[5, :2], n[5] = [7, 8], 2
    ids[7, :2], n[7] = [7, 7], 2
    s, row, out = jref.call(toks, tab, ref.begin(0), [3], ids, n, 16, 1, (9,))
    assert s == (3, True, False, False) and out == [6] and row.tolist() == [1 << 9]
    s, row, out = jref.call(toks, tab, ref.begin(5), [], ids, n, 1, 1, (9,))
    assert s == (6, True, False, False) and out == [7] and row.tolist() == [1 << 8]       # row_len_out 1: the next call goes on
    s, row, out = jref.call(toks, tab, ref.begin(0), [4], ids, n, 16, 1, (9,))
    assert s == (3, True, False, False) and out == [7]                                     # the second "o" does not walk: emission stops
    assert jref.call(toks, tab, ref.FREE, [3], ids, n, 16, 1, (9,))[2] == [] and jref.call(toks, tab, ref.begin(0), [77], ids, n, 16, 1, (9,))[0] == ref.BROKEN


def test_ref_utf8_trim():
    tab = cases.compiled("(é|è)x")
    assert jref.raw_run(tab, 0) == b"\xc3" and jref.run(tab, 0) == b""
    assert jref.run(tab, _state_behind(tab, "é".encode())) == b"x" and jref.run(tab, _state_behind(tab, "è".encode())) == b"x"
    assert jref.run(tab, _state_behind(tab, b"\xc3")) == b""                                # a9 or a8
    tab = cases.compiled("€(a|b)")
    assert jref.run(tab, 0) == "€".encode() and jref.run(tab, _state_behind(tab, b"\xe2")) == b"\x82\xac"       # leading continuation bytes stay
    for data, want in ((b"ab\xc3", b"ab"), (b"ab\xc3\xa9", b"ab\xc3\xa9"), (b"\xe2\x82", b""), (b"\xf0\x9f\x8c", b""), (b"\xf0\x9f\x8c\x8d", b"\xf0\x9f\x8c\x8d"),
                       (b"\xa9x\xc3", b"\xa9x"), (b"\x80\x80", b"\x80\x80"), (b"\xc3\xa9\xe2", b"\xc3\xa9"), (b"\xe2x\x82", b"\xe2x\x82"), (b"\xff\x80\x80", b""),
                       (b"\xc3\x80\x80", b"\xc3\x80\x80"), (b"", b"")):
        assert jref.trim(data) == want, data


def test_ref_cap_cycle_and_accepting_state():
    tab = cases.compiled("a{70}")
    assert ref.n_states(tab) == 71
    assert jref.run(tab, 0) == b"a" * 64
    assert jref.run(tab, _state_behind(tab, b"a" * 64)) == b"a" * 6
    assert jref.run(tab, _state_behind(tab, b"a" * 70)) == b""
    tab = cases.compiled("ab?")
    q = _state_behind(tab, b"a")
    assert tab[1][q] and int((tab[0][q] < ref.n_states(tab)).sum()) == 1 and jref.force(tab, q) is None and jref.run(tab, 0) == b"a"
    cyc = cases.cycle_automaton()
    assert jref.run(cyc, 0) == b"ab" * 32 and jref.run(cyc, 1) == b"ba" * 32
    # the cap first, the trim behind it: 62 bytes and a three-byte character do not fit
    assert jref.run(cases.chain_automaton(b"a" * 62 + "€".encode() + b"b"), 0) == b"a" * 62
    assert jref.run(cases.chain_automaton(b"a" * 61 + "€".encode() + b"b"), 0) == b"a" * 61 + "€".encode()


def test_ref_index_layout():
    assert jref.index_bytes(3) == 3 * 322
    ids = np.arange(2 * 64, dtype=np.uint32).reshape(2, 64)
    buf = jref.pack_index(ids, [5, 200], [1, 2], np.full((2, 64), 7, dtype=np.uint8))
    assert buf.size == 644 and buf.ctypes.data % 4 == 0
    assert buf[:4].tolist() == [0, 0, 0, 0] and buf[4:8].tolist() == [1, 0, 0, 0] and buf[512:516].tolist() == [5, 200, 1, 2] and (buf[516:] == 7).all()
    p = jref.index_parts(buf, 2)
    assert (p[0] == ids).all() and p[1].tolist() == [5, 200] and p[2].tolist() == [1, 2]


# ---------------------------------------------------------------------------------------------- the kernels' code against the definition
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("lanes", LANES)
def test_sim_runs(sim, name, lanes):
    cases.check_runs(runners(sim, name, lanes)[1], name)


def test_sim_runs_4096_states(sim):
    cases.check_runs(runners(sim, "gaps")[1], "gaps", sizes=(4096,))


def test_sim_runs_of_compiled_patterns(sim):
    runs = runners(sim, "gaps")[1]
    for pat in (JSON, TOOL, "(é|è)x", "a{70}", "ab?", r"\d{4}-\d{2}-\d{2}"):
        tab = cases.compiled(pat)
        got, got_len = runs(ref.table_bytes(*tab), ref.n_states(tab))[:2]
        want, want_len = jref.run_arrays(tab)
        assert (got == want).all() and got_len.tolist() == want_len.tolist(), pat


def test_sim_mutant_accept_fails_the_runs_check(sim):
    cases.check_runs(runners(sim, "gaps")[1], "gaps")
    with pytest.raises(AssertionError):
        cases.check_runs(runners(sim, "gaps", mutant="accept")[1], "gaps")


def test_sim_mutant_nowalk_fails_the_adversarial_check(sim):
    cases.check_adversarial(runners(sim, "gaps")[0])
    with pytest.raises(AssertionError):
        cases.check_adversarial(runners(sim, "gaps", mutant="nowalk")[0])


@pytest.mark.parametrize("lanes", LANES)
def test_sim_scatter(sim, lanes):
    rng = np.random.RandomState(3)
    for S in (1, 2, 63, 65):
        n = rng.randint(0, 70, size=S)                                        # (rows above 64 ids: cut at 64, as the index has room for)
        n[rng.randint(0, S)] = 0
        off = np.concatenate([[0], np.cumsum(n)]).astype(np.uint64)
        csr = rng.randint(1, 1 << 31, size=int(off[-1])).astype(np.uint32)
        ids, n_ids = sim.scatter(csr, off, S, lanes=lanes)
        for q in range(S):
            k = min(int(n[q]), 64)
            assert n_ids[q] == k and ids[q, :k].tolist() == csr[int(off[q]):int(off[q]) + k].tolist() and (ids[q, k:] == 0).all()
    # offsets that point behind the CSR are not followed
    ids, n_ids = sim.scatter(np.arange(1, 4, dtype=np.uint32), np.array([0, 2, 9, 5], dtype=np.uint64), 3, cap=3, lanes=lanes)
    assert n_ids.tolist() == [2, 1, 0] and ids[0, :3].tolist() == [1, 2, 0] and ids[1, :2].tolist() == [3, 0]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("lanes", LANES)
def test_sim_jump_against_the_definition(sim, name, lanes):
    cases.check_jump(runners(sim, name, lanes)[0], name, row_lens=(1, 3, 16, 64) if lanes == 64 else (3,))


@pytest.mark.parametrize("lanes", LANES)
def test_sim_adversarial_tables_keep_free_layouts_and_the_zero_index(sim, lanes):
    run, _, step = runners(sim, "gaps", lanes)
    cases.check_adversarial(run)
    cases.check_keep_free_and_layouts(run)
    cases.check_zero_index_is_the_step(run, step)


def test_sim_geometry_matches_the_reference(sim):
    g = sim.geometry()
    assert (g["max_bytes"], g["max_ids"], g["index_bytes_per_state"]) == (jref.MAX_BYTES, jref.MAX_IDS, jref.INDEX_BYTES_PER_STATE) == (64, 64, 322)


# ---------------------------------------------------------------------------------------------- the C ABI's refusals (no device is touched)
@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as entry
    entry.build()
    from splintr_amd import _ffi
    return _ffi


def test_abi_refuses_before_the_device(ffi):
    L = ffi.lib()
    i, o, out, jo = ffi.SplDfaIn(1, 1), ffi.SplDfaOpts(0, 4, (7,)), ffi.SplDfaOut(), ffi.SplDfaJumpOut(16)
    assert L.spl_dfa_jump_device(None, ctypes.byref(i), ctypes.byref(o), ctypes.byref(out), ctypes.byref(jo), None) == SPL_EINVAL
    assert b"spl_dfa_jump_device: null handle" in L.spl_last_error()
    assert L.spl_dfa_jump_index_device(None, None, 1, None, None) == SPL_EINVAL and b"spl_dfa_jump_index_device: null handle" in L.spl_last_error()
    # the existing structs keep their sizes; the new one
    assert ctypes.sizeof(ffi.SplDfaOpts) == 48 and ctypes.sizeof(ffi.SplDfaIn) == 64 and ctypes.sizeof(ffi.SplDfaOut) == 32
    assert ctypes.sizeof(ffi.SplDfaJumpOut) == 32
    hdr = open(ffi.__file__.replace("splintr_amd/_ffi.py", "include/splintr_hip.h")).read()
    assert "#define SPL_DFA_JUMP_MAX_BYTES 64" in hdr and "#define SPL_DFA_JUMP_MAX_IDS   64" in hdr
    assert "#define SPL_DFA_JUMP_INDEX_BYTES(n_states) ((size_t)(n_states) * (64 * 4 + 1 + 1 + 64))" in hdr
    assert (ffi.SPL_DFA_JUMP_MAX_BYTES, ffi.SPL_DFA_JUMP_MAX_IDS) == (jref.MAX_BYTES, jref.MAX_IDS)
    assert ffi.SPL_DFA_JUMP_INDEX_BYTES(11) == jref.index_bytes(11) == 11 * 322
    for sym in ("spl_dfa_jump_index_device", "spl_dfa_jump_device"):
        assert sym in ffi.SYMBOLS and sym + "(" in hdr
