"""Guided choice without a GPU: the definition (tests/choice_ref.py) pinned by hand-worked examples, and the code the kernel runs
(splintr_amd/csrc/spl_k_choice.h, evaluated by tests/hostsim/choice_sim.cpp with 64, 5, 3 and 1 lanes and pieces of 4, 8 and 8 192 words)
against that definition through the checks of tests/choice_cases.py -- one-slot tables of every short string, random tables of 2 .. 64
slots walked along and off their masks, every probe id from every state, END ids, flags, layouts, rows no call writes -- plus two mutants
of the header that a named check must catch, and the C ABI's refusals through the real library."""
import ctypes

import pytest

import choice_cases as cases
import choice_ref as ref

# (lanes, piece words): the hardware's shape; a few lanes a group and many pieces; a binary search per slot; slots in batches
SHAPES = [(64, 8192), (5, 4), (1, 8), (3, 8192), (64, 4)]
NAMES = sorted(cases.TOYS)
SPL_EINVAL = -1


@pytest.fixture(scope="module")
def sim():
    import choice_sim
    choice_sim.lib()
    return choice_sim


def runner(sim, name, lanes=64, piece=8192, mutant="", v4=None):
    vocab, specials = cases.TOYS[name]()
    v = sim.Vocab(vocab, specials)

    def run(table, **kw):
        return sim.run(v, table, lanes=lanes, piece=piece, mutant=mutant, v4=v4, **kw)
    return run


# ---------------------------------------------------------------------------------------------- the definition, by hand
YES = ref.ordinary({0: b"y", 1: b"ye", 2: b"yes", 3: b"yel", 4: b"n", 5: b"no", 6: b"low"})
YES_CHOICES = [b"yes", b"no", b"yellow"]
END = (9,)


def _walk(state, ids, **kw):
    return ref.step(YES, YES_CHOICES, state, ids, END, **kw)


def test_ref_yes_no_yellow():
    s0 = ref.begin(YES_CHOICES)
    # the first mask: every token that begins a choice -- not "low", not END (no remainder is empty)
    assert ref.allowed(YES, YES_CHOICES, s0, END) == {0, 1, 2, 3, 4, 5}
    assert ref.allowed(YES, YES_CHOICES, ref.begin(YES_CHOICES, [1]), END) == {4, 5}
    assert ref.allowed(YES, YES_CHOICES, ref.begin(YES_CHOICES, [0, 2]), END) == {0, 1, 2, 3}
    assert ref.mask(YES, YES_CHOICES, s0, 1, END).tolist() == [0x3F] and ref.mask(YES, YES_CHOICES, ref.FREE, 2, END).tolist() == [0xFFFFFFFF] * 2
    # every path to "yes": y e? -- there is no token "e" or "s" or "es": only ye + ..., yes
    assert _walk(s0, [2]) == (frozenset([0]), 3, False, False, 0)
    assert ref.allowed(YES, YES_CHOICES, _walk(s0, [2]), END) == {9}                    # END only where the remainder is empty
    assert _walk(s0, [2, 9]) == (frozenset(), 3, False, True, 0)
    assert _walk(s0, [0]) == (frozenset([0, 2]), 1, False, False, 0)                    # "y": yes and yellow remain; no token spells "e"
    assert ref.allowed(YES, YES_CHOICES, _walk(s0, [0]), END) == set()
    assert ref.settle(YES, YES_CHOICES, _walk(s0, [0]), END) == ref.BROKEN               # the vocabulary lacks the byte that comes next
    assert _walk(s0, [1]) == (frozenset([0, 2]), 2, False, False, 0) and ref.allowed(YES, YES_CHOICES, _walk(s0, [1]), END) == set()
    # "no": n o? -- no token "o": only the whole "no"; "yellow": yel + low
    assert _walk(s0, [5, 9]) == (frozenset(), 2, False, True, 1)
    assert ref.allowed(YES, YES_CHOICES, _walk(s0, [4]), END) == set()
    assert _walk(s0, [3]) == (frozenset([2]), 3, False, False, 0) and ref.allowed(YES, YES_CHOICES, _walk(s0, [3]), END) == {6}
    assert _walk(s0, [3, 6, 9]) == (frozenset(), 6, False, True, 2)
    # leaving the mask: END too early, a token of another choice, an id that is none; later ids are not read
    assert _walk(s0, [9]) == ref.BROKEN and _walk(s0, [3, 5]) == ref.BROKEN and _walk(s0, [77, 2]) == ref.BROKEN
    assert _walk(s0, [2, 9, 77]) == (frozenset(), 3, False, True, 0)
    assert ref.state_row(_walk(s0, [3])).tolist() == [4, 3] and ref.state_row(_walk(s0, [5, 9])).tolist() == [0, 2 | 1 << 9 | 1 << 16]
    assert ref.state_row(ref.BROKEN).tolist() == [0, 1 << 8] and ref.row_state(ref.raw_row([0, 2], 3)) == (frozenset([0, 2]), 3, False, False, 0)


def test_ref_a_and_ab_with_end_and_then_free():
    toks = ref.ordinary({0: b"a", 1: b"ab", 2: b"b"})
    ch = [b"a", b"ab"]
    s0 = ref.begin(ch)
    a = ref.step(toks, ch, s0, [0], END)
    assert a == (frozenset([0, 1]), 1, False, False, 0)
    assert ref.allowed(toks, ch, a, END) == {2, 9}                                      # go on to "ab", or end "a"
    assert ref.step(toks, ch, a, [9], END) == (frozenset(), 1, False, True, 0)
    assert ref.step(toks, ch, a, [2], END) == (frozenset([1]), 2, False, False, 0)
    assert ref.step(toks, ch, a, [2, 9], END) == (frozenset(), 2, False, True, 1)
    assert ref.step(toks, ch, s0, [1, 9], END) == (frozenset(), 2, False, True, 1)
    # THEN_FREE: "a" ends the sequence at once -- "ab" can only be reached by its own token -- and END ids mean nothing
    assert ref.step(toks, ch, s0, [0, 2], END, then_free=True) == (frozenset(), 1, False, True, 0)
    assert ref.step(toks, ch, s0, [1], END, then_free=True) == (frozenset(), 2, False, True, 1)
    assert ref.step(toks, ch, s0, [9], END, then_free=True) == ref.BROKEN
    assert ref.allowed(toks, ch, s0, END, then_free=True) == {0, 1}


# ---------------------------------------------------------------------------------------------- the kernel's code against the definition
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("lanes, piece", SHAPES)
def test_sim_one_slot_strings(sim, name, lanes, piece):
    for then_free in (False, True):
        for extra in (0, 3):
            cases.check_one_slot_strings(runner(sim, name, lanes, piece), name, then_free, extra)


@pytest.mark.parametrize("mutant, name", [("lcp", "chain"), ("lcp", "gaps"), ("eq", "chain"), ("eq", "gaps")])
def test_sim_mutants_fail_the_one_slot_check(sim, mutant, name):
    cases.check_one_slot_strings(runner(sim, name), name)
    with pytest.raises(AssertionError):
        cases.check_one_slot_strings(runner(sim, name, mutant=mutant), name)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("lanes, piece", SHAPES)
def test_sim_tables_and_walks(sim, name, lanes, piece):
    cases.check_tables_and_walks(runner(sim, name, lanes, piece), name, then_free=(lanes in (5, 3)))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("then_free", [False, True])
def test_sim_every_probe_id_from_every_state(sim, name, then_free):
    lanes, piece = SHAPES[NAMES.index(name) % len(SHAPES)]
    cases.check_every_probe_id_from_every_state(runner(sim, name, lanes, piece), name, then_free)


@pytest.mark.parametrize("lanes, piece", SHAPES)
def test_sim_long_and_edge_choices(sim, lanes, piece):
    cases.check_long_and_edge_choices(lambda name: runner(sim, name, lanes, piece))


@pytest.mark.parametrize("lanes, piece", SHAPES)
def test_sim_end_ids_flags_layout_and_load(sim, lanes, piece):
    run = runner(sim, "gaps", lanes, piece)
    cases.check_end_ids_and_flags(run)
    cases.check_layout(run)
    cases.check_load_sanitation(run)
    cases.check_layout(runner(sim, "gaps", lanes, piece, v4=False))                    # word stores where 16-byte stores would do


def test_sim_geometry_matches_the_reference(sim):
    g = sim.geometry()
    assert (g["slots"], g["max_len"], g["table_bytes"], g["state_words"], g["max_end"]) == (ref.SLOTS, ref.MAX_LEN, ref.TABLE_BYTES, ref.STATE_WORDS, ref.MAX_END)
    assert g["piece"] == 8192 and g["wave"] == 64


# ---------------------------------------------------------------------------------------------- the C ABI's refusals (no device is touched)
@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as entry
    entry.build()
    from splintr_amd import _ffi
    return _ffi


def test_abi_refuses_before_the_device(ffi):
    L = ffi.lib()
    i, o, out = ffi.SplChoiceIn(1, 1), ffi.SplChoiceOpts(0, 4, (7,)), ffi.SplChoiceOut()
    assert L.spl_choice_step_device(None, ctypes.byref(i), ctypes.byref(o), ctypes.byref(out), None) == SPL_EINVAL
    assert b"spl_choice_step_device: null handle" in L.spl_last_error()
    assert L.spl_choice_reserve_device(None) == SPL_EINVAL and b"spl_choice_reserve_device: null handle" in L.spl_last_error()
    assert ctypes.sizeof(ffi.SplChoiceOpts) == 48 and ctypes.sizeof(ffi.SplChoiceIn) == 48 and ctypes.sizeof(ffi.SplChoiceOut) == 32
    assert (ffi.SPL_CHOICE_THEN_FREE, ffi.SPL_CHOICE_KEEP_FREE, ffi.SPL_CHOICE_I64) == (ref.THEN_FREE, ref.KEEP_FREE, ref.I64) == (1, 2, 4)
    hdr = open(ffi.__file__.replace("splintr_amd/_ffi.py", "include/splintr_hip.h")).read()
    for name, val in (("SPL_CHOICE_SLOTS", "64"), ("SPL_CHOICE_MAX_LEN", "64"), ("SPL_CHOICE_TABLE_BYTES", "(64 * 64 + 64)"), ("SPL_CHOICE_STATE_WORDS", "2"),
                      ("SPL_CHOICE_MAX_END", "8")):
        assert "#define %s %s%s" % (name, " " * (22 - len(name)), val) in hdr, name
        assert getattr(ffi, name) == eval(val)
    assert '"choice_piece_words"' in hdr
