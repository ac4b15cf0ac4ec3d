"""The regex guide without a GPU: the definition (tests/dfa_ref.py) pinned by hand-worked examples, and the code the kernels run
(splintr_amd/csrc/spl_k_dfa.h, evaluated by tests/hostsim/dfa_sim.cpp with 64, 5, 3 and 1 lanes) against that definition through the
checks of tests/dfa_cases.py -- the index bit for bit, the cross-check against guided choice, every probe id from every state, END ids,
flags, layouts, words no call writes -- plus two mutants of the header that a named check must catch, and the C ABI's refusals through
the real library."""
import ctypes

import numpy as np
import pytest

import choice_ref
import dfa_cases as cases
import dfa_ref as ref

# (lanes of the step, lanes of the index build, states a block): the hardware's shape; ids in turns and states in small batches
SHAPES = [(64, 64, 256), (5, 5, 7), (3, 3, 64), (1, 1, 2)]
NAMES = sorted(cases.TOYS)
SPL_EINVAL = -1


@pytest.fixture(scope="module")
def sim():
    import dfa_sim
    dfa_sim.lib()
    return dfa_sim


def runners(sim, name, lanes=64, ilanes=64, s_block=256, mutant="", v4=None):
    vocab, specials = cases.TOYS[name]()
    v = sim.Vocab(vocab, specials)

    def run(table, n_states, **kw):
        return sim.run(v, table, n_states, lanes=lanes, mutant=mutant, v4=v4, **kw)

    def index(table, n_states, n_words):
        return sim.index(v, table, n_states, n_words, lanes=ilanes, s_block=s_block, mutant=mutant)
    return run, index


# ---------------------------------------------------------------------------------------------- the definition, by hand
YES_VOCAB = {0: b"y", 1: b"ye", 2: b"yes", 3: b"yel", 4: b"n", 5: b"no", 6: b"low"}
YES = ref.ordinary(YES_VOCAB)
YES_CHOICES = [b"yes", b"no", b"yellow"]
END = (9,)


def _yes_table():
    """yes|no|yellow by hand: 0 -y-> 1 -e-> 2 -s-> 3* ; 2 -l-> 4 -l-> 5 -o-> 6 -w-> 3* ; 0 -n-> 7 -o-> 3*   (3 accepts)"""
    t = np.full((8, 256), ref.DEAD, dtype=np.uint16)
    for q, x, to in ((0, "y", 1), (1, "e", 2), (2, "s", 3), (2, "l", 4), (4, "l", 5), (5, "o", 6), (6, "w", 3), (0, "n", 7), (7, "o", 3)):
        t[q, ord(x)] = to
    return t, np.array([0, 0, 0, 1, 0, 0, 0, 0], dtype=np.uint8)


def test_ref_yes_no_yellow_shows_the_choice_rule_sets():
    tab = _yes_table()
    s0 = ref.begin(0)
    c0 = choice_ref.begin(YES_CHOICES)
    # the same allowed sets as guided choice at every state: {0 .. 5} at the start, {9} behind "yes", broken behind "y"
    assert ref.allowed(YES, tab, s0, END) == choice_ref.allowed(YES, YES_CHOICES, c0, END) == {0, 1, 2, 3, 4, 5}
    yes = ref.step(YES, tab, s0, [2], END)
    assert yes == (3, True, False, False) and ref.allowed(YES, tab, yes, END) == {9}
    assert choice_ref.allowed(YES, YES_CHOICES, choice_ref.step(YES, YES_CHOICES, c0, [2], END), END) == {9}
    y = ref.step(YES, tab, s0, [0], END)
    assert y == (1, True, False, False) and ref.allowed(YES, tab, y, END) == set() and ref.settle(YES, tab, y, END) == ref.BROKEN
    assert choice_ref.settle(YES, YES_CHOICES, choice_ref.step(YES, YES_CHOICES, c0, [0], END), END) == choice_ref.BROKEN
    for ids in ([1], [3], [4], [5], [3, 6], [2, 9], [5, 9], [3, 6, 9], [9], [3, 5], [77, 2], [2, 9, 77]):
        d = ref.settle(YES, tab, ref.step(YES, tab, s0, ids, END), END)
        c = choice_ref.settle(YES, YES_CHOICES, choice_ref.step(YES, YES_CHOICES, c0, ids, END), END)
        assert (d[1], d[2], d[3]) == (bool(c[0]), c[2], c[3]), ids
        assert ref.mask(YES, tab, d, 1, END).tolist() == choice_ref.mask(YES, YES_CHOICES, c, 1, END).tolist(), ids
    assert ref.mask(YES, tab, s0, 1, END).tolist() == [0x3F] and ref.mask(YES, tab, ref.FREE, 2, END).tolist() == [0xFFFFFFFF] * 2
    assert ref.step(YES, tab, s0, [3]) == (4, True, False, False) and ref.allowed(YES, tab, (4, True, False, False), END) == {6}
    assert ref.step(YES, tab, s0, [3, 6, 9], END) == (3, False, False, True)
    # the words
    assert ref.state_row(s0) == 1 << 16 and ref.state_row(yes) == 3 | 1 << 16 and ref.state_row((3, False, False, True)) == 3 | 1 << 18
    assert ref.state_row(ref.BROKEN) == 1 << 17 and ref.state_row(ref.FREE) == 0
    assert ref.row_state(5 | 1 << 16) == (5, True, False, False) and ref.load(tab, (8, True, False, False)) == ref.BROKEN
    assert ref.load(tab, (2, True, True, True)) == ref.BROKEN and ref.load(tab, (2, True, False, True)) == (2, False, False, True)
    # a value that is no state is DEAD, whatever it is; the index by hand
    t2 = tab[0].copy()
    t2[0, ord("q")] = 8
    t2[0, ord("r")] = 0x1234
    assert ref.walk((t2, tab[1]), 0, b"q") == ref.DEAD and ref.walk((t2, tab[1]), 0, b"r") == ref.DEAD and ref.walk(tab, 0, b"yel") == 4
    rows, some = ref.index(YES, tab, 1)
    assert rows.shape == (8, 4) and rows[:, 0].tolist() == [0x3F, 0, 0, 0, 1 << 6, 0, 0, 0] and some.tolist() == [1, 0, 0, 0, 1, 0, 0, 0]
    # the compiler's automaton of the same language is this one up to the numbering
    ctab = cases.alternation(YES_CHOICES)
    assert ref.n_states(ctab) == 8 and ref.allowed(YES, ctab, ref.begin(0), END) == {0, 1, 2, 3, 4, 5}


def test_ref_a_and_ab_with_end():
    toks = ref.ordinary({0: b"a", 1: b"ab", 2: b"b"})
    t = np.full((3, 256), ref.DEAD, dtype=np.uint16)
    t[0, ord("a")], t[1, ord("b")] = 1, 2
    tab = (t, np.array([0, 1, 1], dtype=np.uint8))
    s0 = ref.begin(0)
    a = ref.step(toks, tab, s0, [0], END)
    assert a == (1, True, False, False)
    assert ref.allowed(toks, tab, a, END) == {2, 9}                                     # go on to "ab", or end "a"
    assert ref.step(toks, tab, a, [9], END) == (1, False, False, True)
    assert ref.step(toks, tab, a, [2], END) == (2, True, False, False)
    assert ref.step(toks, tab, a, [2, 9], END) == (2, False, False, True)
    assert ref.step(toks, tab, s0, [1, 9], END) == (2, False, False, True)
    assert ref.allowed(toks, tab, (2, True, False, False), END) == {9} and ref.allowed(toks, tab, s0, END) == {0, 1}
    assert ref.step(toks, tab, s0, [9], END) == ref.BROKEN and ref.step(toks, tab, s0, [2], END) == ref.BROKEN
    # END as an ordinary id that also walks on: the ordinary rule wins
    assert ref.step(toks, tab, a, [2], (2,)) == (2, True, False, False) and ref.step(toks, tab, a, [2, 2], (2,)) == (2, False, False, True)
    assert ref.call(toks, tab, a, [], 1, END)[1].tolist() == [1 << 2 | 1 << 9]


# ---------------------------------------------------------------------------------------------- the kernels' code against the definition
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("lanes, ilanes, s_block", SHAPES)
def test_sim_index(sim, name, lanes, ilanes, s_block):
    _, index = runners(sim, name, lanes, ilanes, s_block)
    cases.check_index(index, name, extra_words=(0, 1, 3))


def test_sim_index_4096_states(sim):
    _, index = runners(sim, "gaps")
    cases.check_index(index, "gaps", sizes=(4096,))


@pytest.mark.parametrize("name", NAMES)
def test_sim_mutant_first_fails_the_index_check(sim, name):
    cases.check_index(runners(sim, name)[1], name)
    with pytest.raises(AssertionError):
        cases.check_index(runners(sim, name, mutant="first")[1], name)


def test_sim_mutant_end_fails_the_end_check(sim):
    cases.check_end_ids(runners(sim, "gaps")[0])
    with pytest.raises(AssertionError):
        cases.check_end_ids(runners(sim, "gaps", mutant="end")[0])


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("lanes, ilanes, s_block", SHAPES)
def test_sim_against_guided_choice(sim, name, lanes, ilanes, s_block):
    cases.check_against_choice(runners(sim, name, lanes)[0], name, steps=6 if lanes != 64 else 8)


@pytest.mark.parametrize("name", NAMES)
def test_sim_every_probe_id_from_every_state(sim, name):
    lanes = SHAPES[NAMES.index(name) % len(SHAPES)][0]
    cases.check_every_probe_id_from_every_state(runners(sim, name, lanes)[0], name)


@pytest.mark.parametrize("lanes, ilanes, s_block", SHAPES)
def test_sim_end_ids_flags_layout_and_load(sim, lanes, ilanes, s_block):
    run, index = runners(sim, "gaps", lanes, ilanes, s_block)
    cases.check_end_ids(run)
    cases.check_flags(run)
    cases.check_layout_and_load(run, index)
    run, index = runners(sim, "gaps", lanes, ilanes, s_block, v4=False)             # word accesses where 16-byte accesses would do
    cases.check_layout_and_load(run, index)


def test_sim_geometry_matches_the_reference(sim):
    g = sim.geometry()
    assert (g["dead"], g["max_states"], g["state_words"], g["max_end"]) == (ref.DEAD, ref.MAX_STATES, ref.STATE_WORDS, ref.MAX_END)
    assert (g["keep_free"], g["i64"]) == (ref.KEEP_FREE, ref.I64) and g["wave"] == 64


# ---------------------------------------------------------------------------------------------- the C ABI's refusals (no device is touched)
@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as entry
    entry.build()
    from splintr_amd import _ffi
    return _ffi


def test_abi_refuses_before_the_device(ffi):
    L = ffi.lib()
    i, o, out = ffi.SplDfaIn(1, 1), ffi.SplDfaOpts(0, 4, (7,)), ffi.SplDfaOut()
    assert L.spl_dfa_step_device(None, ctypes.byref(i), ctypes.byref(o), ctypes.byref(out), None) == SPL_EINVAL
    assert b"spl_dfa_step_device: null handle" in L.spl_last_error()
    assert L.spl_dfa_index_device(None, None, 1, 1, None, None) == SPL_EINVAL and b"spl_dfa_index_device: null handle" in L.spl_last_error()
    assert L.spl_dfa_reserve_device(None) == SPL_EINVAL and b"spl_dfa_reserve_device: null handle" in L.spl_last_error()
    assert ctypes.sizeof(ffi.SplDfaOpts) == 48 and ctypes.sizeof(ffi.SplDfaIn) == 64 and ctypes.sizeof(ffi.SplDfaOut) == 32
    assert (ffi.SPL_DFA_KEEP_FREE, ffi.SPL_DFA_I64) == (ref.KEEP_FREE, ref.I64) == (2, 4)
    hdr = open(ffi.__file__.replace("splintr_amd/_ffi.py", "include/splintr_hip.h")).read()
    for name, val in (("SPL_DFA_DEAD", "0xFFFF"), ("SPL_DFA_MAX_STATES", "4096"), ("SPL_DFA_STATE_WORDS", "1"), ("SPL_DFA_MAX_END", "8")):
        assert "#define %s %s%s" % (name, " " * (19 - len(name)), val) in hdr, name
        assert getattr(ffi, name) == eval(val) == getattr(ref, name[8:])
    assert "#define SPL_DFA_TABLE_BYTES(n_states) ((size_t)(n_states) * 512 + (size_t)(n_states))" in hdr
    assert "#define SPL_DFA_INDEX_BYTES(n_states, n_words) ((size_t)(n_states) * ((((size_t)(n_words) + 3) & ~(size_t)3) * 4 + 1))" in hdr
    assert ffi.SPL_DFA_TABLE_BYTES(11) == 11 * 513 and ffi.SPL_DFA_INDEX_BYTES(3, 5) == 3 * 33 and ffi.SPL_DFA_INDEX_BYTES(2, 8) == 2 * 33
