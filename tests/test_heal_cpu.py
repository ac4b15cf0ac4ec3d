"""Token healing without a GPU: the definition (tests/heal_ref.py) pinned by hand-worked examples, and the code the kernels run
(splintr_amd/csrc/spl_k_heal.h, evaluated by tests/hostsim/heal_sim.cpp with 64, 5, 3 and 1 lanes) against that definition -- every prefix
of 1 .. 5 bytes of {a, b, c} on three toy vocabularies, steps fed at every cut, begin over every limit -- plus two mutants of the header
that named checks must catch, and the C ABI's refusals through the real library."""
import ctypes

import numpy as np
import pytest

import heal_cases as cases
import heal_ref as ref

LANES = [64, 5, 3, 1]
SPL_EINVAL = -1


@pytest.fixture(scope="module")
def sim():
    import heal_sim
    heal_sim.lib()
    return heal_sim


# ---------------------------------------------------------------------------------------------- the definition, by hand
HTTP = ref.ordinary({0: b"http", 1: b":", 2: b"://", 3: b"http://", 4: b"h", 5: b"ht", 6: b"/", 7: b"x"})


def test_ref_http_family():
    # P = ":" -- covering ":" and "://"; nothing is a proper prefix of a single byte
    assert ref.allowed(HTTP, b":") == {1, 2}
    # P = "http:" -- covering "http://" alone; partial h, ht, http
    assert ref.allowed(HTTP, b"http:") == {3, 0, 4, 5}
    # auto: ":" is taken because "://" extends it; "http" is taken too because "http://" extends "http:"
    assert ref.begin(HTTP, [7, 0, 1], max_back=3, auto=True) == (2, b"http:")
    # ... "x" is not: nothing extends "xhttp:"
    assert ref.begin(HTTP, [7, 0, 1], max_back=1, auto=True) == (1, b":")
    # without "http://" nothing extends "http:": only ":" is taken
    assert ref.begin([t for t in HTTP if t[0] != 3], [7, 0, 1], max_back=3, auto=True) == (1, b":")
    # plain: exactly as many as the limits allow
    assert ref.begin(HTTP, [7, 0, 1], max_back=3) == (3, b"xhttp:")
    assert ref.begin(HTTP, [7, 0, 1], max_back=2) == (2, b"http:")
    # the steps: "ht" is partial, "h" disagrees with "tp:"
    assert ref.step(HTTP, (b"http:", False, False), [5]) == (b"tp:", False, False)
    assert ref.step(HTTP, (b"http:", False, False), [5, 4]) == (b"", True, False)
    assert ref.step(HTTP, (b"http:", False, False), [3, 7]) == (b"", False, True)


def test_ref_partial_chain_and_uncovered():
    toks = ref.ordinary({0: b"a", 1: b"aa", 2: b"aaa", 3: b"b"})
    assert ref.allowed(toks, b"aaa") == {0, 1, 2}
    assert ref.allowed(toks, b"aab") == {0, 1}                 # nothing covers it: partial a, aa
    assert ref.allowed(toks, b"c") == set()                    # a prefix that nothing covers and nothing begins
    assert ref.mask_words(toks, b"c", 2).tolist() == [0, 0]
    assert ref.mask_words(toks, b"", 2).tolist() == [0xFFFFFFFF] * 2
    assert ref.mask_words(toks, b"aab", 2).tolist() == [3, 0]
    assert ref.step(toks, (b"aab", False, False), [1, 3]) == (b"", False, True)
    assert ref.step(toks, (b"aab", False, False), [0, 0, 0]) == (b"", True, False)      # the third a disagrees with "b"
    assert ref.step(toks, (b"", False, False), [99]) == (b"", False, False)             # free stays free, whatever the id


def test_ref_broken_min_keep_special():
    toks = ref.ordinary({0: b"a", 1: b"ab", 2: b""})            # id 2 has no bytes: not ordinary; id 5 is a special: not in the list
    assert ref.step(toks, (b"ab", False, False), [5]) == (b"", True, False)
    assert ref.step(toks, (b"ab", False, False), [2]) == (b"", True, False)
    assert ref.step(toks, (b"ab", False, True), [0, 5]) == (b"", True, True)            # the bits are sticky
    assert ref.begin(toks, [0, 1, 0], max_back=8) == (3, b"aaba")
    assert ref.begin(toks, [0, 1, 0], max_back=8, min_keep=2) == (1, b"a")
    assert ref.begin(toks, [0, 1, 0], max_back=8, min_keep=3) == (0, b"")
    assert ref.begin(toks, [0, 1, 5], max_back=8) == (0, b"")                            # a special as the last token
    assert ref.begin(toks, [0, 5, 1], max_back=8) == (1, b"ab")
    assert ref.begin(toks, [], max_back=8) == (0, b"")
    row = ref.state_row((b"ab", True, False))
    assert row.tolist() == [2 | 0x100, 0x6261, 0, 0, 0, 0, 0, 0, 0] and ref.row_state(row) == (b"ab", True, False)


# ---------------------------------------------------------------------------------------------- the kernels' code against the definition
def toy(name):
    vocab, specials = cases.TOYS[name]()
    return vocab, specials, ref.ordinary(vocab)


def check_masks(sim, v, toks, ps, got, n_words):
    """NAMED CHECK (the mutants must fail here): every mask row is the definition's."""
    for p, row in zip(ps, got):
        assert row.tolist() == ref.mask_words(toks, p, n_words).tolist(), p


@pytest.mark.parametrize("name", sorted(cases.TOYS))
@pytest.mark.parametrize("lanes", LANES)
def test_sim_masks_of_every_prefix(sim, name, lanes):
    vocab, specials, toks = toy(name)
    v = sim.Vocab(vocab, specials)
    ps = [b""] + cases.prefixes(name)
    for n_words in (v.min_words, v.min_words + 3):
        r = sim.run(v, begin=False, ids=np.zeros((len(ps), 0), dtype=np.int32), state=cases.state_rows(ps), lanes=lanes, n_words=n_words)
        check_masks(sim, v, toks, ps, r["mask"], n_words)
        assert r["live"].tolist() == [int(len(p) > 0) for p in ps]
        assert r["n"].tolist() == [len(ps) - 1, 0]
        assert (r["state"] == cases.state_rows(ps)).all()                        # K = 0 only writes masks
    if name == "chain":
        assert r["max_part"] >= 3


@pytest.mark.parametrize("mutant, name", [("hi", "chain"), ("lcp", "chain"), ("lcp", "gaps")])
def test_sim_mutants_fail_the_mask_check(sim, mutant, name):
    vocab, specials, toks = toy(name)
    v = sim.Vocab(vocab, specials)
    ps = cases.prefixes(name)
    r = sim.run(v, begin=False, ids=np.zeros((len(ps), 0), dtype=np.int32), state=cases.state_rows(ps), mutant=mutant)
    with pytest.raises(AssertionError):
        check_masks(sim, v, toks, ps, r["mask"], v.min_words)


@pytest.mark.parametrize("name", sorted(cases.TOYS))
@pytest.mark.parametrize("lanes", LANES)
def test_sim_one_step_with_every_id(sim, name, lanes):
    vocab, specials, toks = toy(name)
    v = sim.Vocab(vocab, specials)
    pool = cases.probe_ids(vocab, specials)
    ps = [b""] + cases.prefixes(name)[:120] + (cases.EDGE_PREFIXES if name == "edges" else [])
    pairs = [(p, t) for p in ps for t in pool]
    ids = np.array([[t] for _, t in pairs], dtype=np.uint32).view(np.int32)
    r = sim.run(v, begin=False, ids=ids, state=cases.state_rows([p for p, _ in pairs]), lanes=lanes)
    broke = 0
    for (p, t), row, m in zip(pairs, r["state"], r["mask"]):
        want = ref.step(toks, (p, False, False), [t])
        assert row.tolist() == ref.state_row(want).tolist(), (p, t)
        assert m.tolist() == ref.mask_words(toks, want[0], v.min_words).tolist(), (p, t)
        broke += want[1]
    assert r["n"].tolist() == [int(r["live"].sum()), broke]


@pytest.mark.parametrize("name", sorted(cases.TOYS))
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_sim_steps_at_every_cut(sim, name, dtype):
    """The same ids fed all at once, one at a time and at every two-way cut: equal state rows bit for bit, equal to the definition's."""
    vocab, specials, toks = toy(name)
    v = sim.Vocab(vocab, specials)
    sc = cases.step_cases(name)
    ps, seqs = [p for p, _ in sc], [ids for _, ids in sc]
    K = len(seqs[0])
    want = np.stack([ref.state_row(ref.step(toks, (p, False, False), ids)) for p, ids in sc])
    assert any(ref.row_state(w)[2] for w in want) and any(ref.row_state(w)[1] for w in want)       # some heal, some break
    feed = lambda st, part, **kw: sim.run(v, begin=False, ids=cases.rows_of(part, max(len(part[0]), 1), dtype)[0][:, :len(part[0])],
                                          state=st, **kw)
    whole = feed(cases.state_rows(ps), seqs)
    assert (whole["state"] == want).all()
    for m, w in zip(whole["mask"], want):
        assert m.tolist() == ref.mask_words(toks, ref.row_state(w)[0], v.min_words).tolist()
    st = cases.state_rows(ps)
    for k in range(K):
        st = feed(st, [s[k:k + 1] for s in seqs], in_place=(k % 2 == 0), lanes=5)["state"]
    assert (st == want).all()
    for cut in range(1, K):
        a = feed(cases.state_rows(ps), [s[:cut] for s in seqs], lanes=3)["state"]
        b = feed(a, [s[cut:] for s in seqs], lanes=1)
        assert (b["state"] == want).all() and (b["mask"] == whole["mask"]).all()
    # lengths: only the first len[b] entries of a row count
    rows, _ = cases.rows_of(seqs, K, dtype)
    lens = np.array([i % (K + 2) - 1 for i in range(len(seqs))], dtype=np.int32)      # -1 .. K: clamped to 0 .. K
    r = sim.run(v, begin=False, ids=rows, lengths=lens, state=cases.state_rows(ps))
    for (p, ids), n, row in zip(sc, lens, r["state"]):
        assert row.tolist() == ref.state_row(ref.step(toks, (p, False, False), ids[:max(int(n), 0)])).tolist()


def test_sim_int64_values_that_are_no_ids(sim):
    vocab, specials, toks = toy("gaps")
    v = sim.Vocab(vocab, specials)
    bad = [-1, -100, 1 << 32, (1 << 32) + 2, -(1 << 63)]
    r = sim.run(v, begin=False, ids=np.array([[x] for x in bad], dtype=np.int64), state=cases.state_rows([b"ab"] * len(bad)))
    assert all(ref.row_state(row) == (b"", True, False) for row in r["state"]) and r["n"].tolist() == [0, len(bad)]
    r = sim.run(v, begin=True, ids=np.array([[2, x] for x in bad], dtype=np.int64), max_back=4)
    assert r["n_back"].tolist() == [0] * len(bad)


def test_sim_keep_free_leaves_free_rows_alone(sim):
    vocab, specials, toks = toy("gaps")
    v = sim.Vocab(vocab, specials)
    ps = [b"", b"ab", b"", b"c", b"zz", b""]
    init = np.arange(len(ps) * v.min_words, dtype=np.uint32).reshape(len(ps), -1) + 77
    ids = np.array([[0], [3], [0], [0], [0], [0]], dtype=np.int32)                   # "abc" heals row 1; "a" breaks rows 3 and 4
    r = sim.run(v, begin=False, ids=ids, state=cases.state_rows(ps), flags=sim.KEEP_FREE, mask_init=init)
    assert r["live"].tolist() == [0] * len(ps) and (r["mask"] == init).all() and r["n"].tolist() == [0, 2]
    r = sim.run(v, begin=False, ids=ids[:, :0], state=cases.state_rows(ps), flags=sim.KEEP_FREE, mask_init=init)
    for p, row, keep in zip(ps, r["mask"], init):
        assert row.tolist() == (ref.mask_words(toks, p, v.min_words).tolist() if p else keep.tolist())


@pytest.mark.parametrize("lanes", LANES)
def test_sim_long_prefixes_and_long_covering_tokens(sim, lanes):
    vocab, specials = cases.vocab_long()
    toks = ref.ordinary(vocab)
    v = sim.Vocab(vocab, specials)
    ps = [b"a", b"a" * 63, b"a" * 64, b"a" * 63 + b"b", b"a" * 62 + b"b", b"b", b"a" * 33]
    r = sim.run(v, begin=False, ids=np.zeros((len(ps), 0), dtype=np.int32), state=cases.state_rows(ps), lanes=lanes)
    check_masks(sim, v, toks, ps, r["mask"], v.min_words)
    assert r["max_part"] == 63                                                      # |P| = 64: a .. a^63
    assert ref.allowed(toks, b"a" * 64) == set(range(66))                            # a^64, a^65 and a^128 cover it
    # the 128-byte token heals a 64-byte prefix; a^63 leaves one byte; begin stops where the prefix would pass 64 bytes
    ids = np.array([[65, 0], [62, 64], [62, 67]], dtype=np.int32)                 # a^128 | a^63 a^65 | a^63 b
    r = sim.run(v, begin=False, ids=ids, state=cases.state_rows([b"a" * 64] * 3), lanes=lanes)
    assert [ref.row_state(x) for x in r["state"]] == [(b"", False, True), (b"", False, True), (b"", True, False)]
    prompts = [[31, 31, 0], [31, 31], [63, 0], [64, 0], [65]]                        # a^32 a^32 a | a^32 a^32 | a^64 a | a^65 a | a^128
    rows, lens = cases.rows_of(prompts, 3, np.int32)
    r = sim.run(v, begin=True, ids=rows, lengths=lens, max_back=8, lanes=lanes)
    assert r["n_back"].tolist() == [2, 2, 1, 1, 0]
    for pr, nb, row, m in zip(prompts, r["n_back"], r["state"], r["mask"]):
        want = ref.begin(toks, pr, max_back=8)
        assert (int(nb), ref.row_state(row)) == (want[0], (want[1], False, False))
        assert m.tolist() == ref.mask_words(toks, want[1], v.min_words).tolist()


@pytest.mark.parametrize("name", sorted(cases.TOYS))
@pytest.mark.parametrize("auto", [False, True])
def test_sim_begin_over_every_limit(sim, name, auto):
    vocab, specials, toks = toy(name)
    v = sim.Vocab(vocab, specials)
    prompts = cases.prompts(name)
    n = 0
    for max_back in range(9):
        for side, dtype, min_keep, lanes in [("right", np.int32, 0, 64), ("left", np.int64, 1, 5), ("right", np.int64, 2, 1), ("left", np.int32, 0, 3)]:
            rows, lens = cases.rows_of(prompts, 8, dtype, side)
            flags = (sim.AUTO if auto else 0) | (sim.PAD_LEFT if side == "left" else 0)
            r = sim.run(v, begin=True, ids=rows, lengths=lens, flags=flags, max_back=max_back, min_keep=min_keep, lanes=lanes)
            for pr, nb, row, m in zip(prompts, r["n_back"], r["state"], r["mask"]):
                want = ref.begin(toks, pr, max_back=max_back, min_keep=min_keep, auto=auto)
                assert (int(nb), ref.row_state(row)) == (want[0], (want[1], False, False)), (pr, max_back, min_keep, side)
                assert m.tolist() == ref.mask_words(toks, want[1], v.min_words).tolist()
                n += want[0]
            assert r["n"].tolist() == [int(r["live"].sum()), 0]
    assert n > 0
    # no lengths: every entry of a row is valid
    full = [p for p in prompts if len(p) == 4][:10] or [prompts[0][:4]]
    rows, _ = cases.rows_of(full, len(full[0]), np.int32)
    r = sim.run(v, begin=True, ids=rows, flags=sim.AUTO if auto else 0, max_back=3)
    assert r["n_back"].tolist() == [ref.begin(toks, p, max_back=3, auto=auto)[0] for p in full]


def test_sim_table_build_refuses_many_equal_byte_strings(sim):
    v = sim.Vocab({i: b"a" for i in range(70)})
    with pytest.raises(AssertionError):
        sim.run(v, begin=False, ids=np.zeros((1, 0), dtype=np.int32), state=cases.state_rows([b"ab"]))
    # a few ids with equal bytes are all of them partial, all of them covering
    vocab = {0: b"a", 1: b"a", 2: b"ab", 3: b"ab", 4: b"b"}
    r = sim.run(sim.Vocab(vocab), begin=False, ids=np.zeros((3, 0), dtype=np.int32), state=cases.state_rows([b"a", b"ab", b"abc"]))
    assert r["mask"][:, 0].tolist() == [0b1111, 0b1111, 0b1111]
    assert [ref.allowed(ref.ordinary(vocab), p) for p in (b"a", b"ab", b"abc")] == [{0, 1, 2, 3}] * 3


# ---------------------------------------------------------------------------------------------- the C ABI's refusals (no device is touched)
@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as entry
    entry.build()
    from splintr_amd import _ffi
    return _ffi


def test_abi_refuses_before_the_device(ffi):
    L = ffi.lib()
    i, o, out = ffi.SplHealIn(1, 1), ffi.SplHealOpts(0, 4), ffi.SplHealOut()
    for fn in (L.spl_heal_begin_device, L.spl_heal_step_device):
        assert fn(None, ctypes.byref(i), ctypes.byref(o), ctypes.byref(out), None) == SPL_EINVAL
        assert b"null handle" in L.spl_last_error()
    assert L.spl_heal_reserve_device(None, 4) == SPL_EINVAL and b"spl_heal_reserve_device: null handle" in L.spl_last_error()
    assert ctypes.sizeof(ffi.SplHealOpts) == 20 and ctypes.sizeof(ffi.SplHealIn) == 40 and ctypes.sizeof(ffi.SplHealOut) == 48
    assert (ffi.SPL_HEAL_AUTO, ffi.SPL_HEAL_KEEP_FREE, ffi.SPL_HEAL_I64, ffi.SPL_HEAL_PAD_LEFT) == (1, 2, 4, 8)
    hdr = open(ffi.__file__.replace("splintr_amd/_ffi.py", "include/splintr_hip.h")).read()
    for name, val in (("SPL_HEAL_STATE_WORDS", 9), ("SPL_HEAL_MAX_PREFIX", 64), ("SPL_HEAL_MAX_BACK", 8)):
        assert "#define %s %s%d" % (name, " " * (20 - len(name)), val) in hdr and getattr(ffi, name) == val
