"""The nest guide (JSON mode) without a GPU: the definition (tests/nest_ref.py) pinned by a hand-worked example, and the code the kernels
run (splintr_amd/csrc/spl_k_nest.h, evaluated by tests/hostsim/nest_sim.cpp with 64, 5, 3 and 1 lanes) against that definition through
the checks of tests/nest_cases.py -- the ops-zero anchor (every check of tests/dfa_cases.py routed through the nest calls), random tables
bit for bit, dep lists entry for entry, the stack and the state row, END and the depth, flags and layouts -- plus three mutants of the
header that a named check must catch, and the C ABI's refusals through the real library."""
import ctypes

import numpy as np
import pytest

import dfa_cases
import dfa_ref
import nest_cases as cases
import nest_ref as ref

# (lanes of the step, lanes of the index build, states a block): the hardware's shape; ids in turns and states in small batches
SHAPES = [(64, 64, 256), (5, 5, 7), (3, 3, 64), (1, 1, 2)]
SPL_EINVAL = -1


@pytest.fixture(scope="module")
def sim():
    import nest_sim
    nest_sim.lib()
    return nest_sim


_vocabs = {}


def runners(sim, name, lanes=64, ilanes=64, s_block=256, mutant="", v4=None):
    if name not in _vocabs:
        vocab, specials, _ = cases.vocab(name)
        _vocabs[name] = sim.Vocab(vocab, specials)
    v = _vocabs[name]

    def run(table, n_states, n_ret, **kw):
        return sim.run(v, table, n_states, n_ret, lanes=lanes, mutant=mutant, v4=v4, **kw)

    def index(table, n_states, n_ret, n_words, dep_cap=None):
        return sim.index(v, table, n_states, n_ret, n_words, dep_cap=dep_cap, lanes=ilanes, s_block=s_block, mutant=mutant)
    return run, index


# ---------------------------------------------------------------------------------------------- the definition, by hand
PAREN = ref.ordinary(cases.vocab_paren()[0])                        # 0 "("  1 ")"  2 "))"  3 "()"  4 "a)"  5 "a"
END = (9,)


def test_ref_paren_table_by_hand():
    tab = cases.paren_table()
    s0 = ref.begin(0)
    # depth 0: "(" opens, "()" opens and closes inside itself (back through symbol 0: state 2), ")" has nothing to pop
    assert ref.allowed(PAREN, tab, s0, END) == {0, 3, 5}
    assert ref.step(PAREN, tab, s0, [1], END) == ref.BROKEN and ref.step(PAREN, tab, s0, [4], END) == ref.BROKEN
    assert ref.step(PAREN, tab, s0, [3], END) == (2, True, False, False, ())
    assert ref.step(PAREN, tab, s0, [5, 5, 0], END) == (1, True, False, False, (0,))
    one = ref.begin(1, (0,))
    assert ref.allowed(PAREN, tab, one, END) == {0, 1, 3, 4, 5}                # "))" closes one bracket too many; END: the stack is not empty
    assert ref.step(PAREN, tab, one, [0], END) == (1, True, False, False, (0, 1))
    assert ref.step(PAREN, tab, one, [4], END) == (2, True, False, False, ())
    assert ref.step(PAREN, tab, one, [2], END) == ref.BROKEN and ref.step(PAREN, tab, one, [9], END) == ref.BROKEN
    # the return state of a pop depends on the popped symbol: 1 goes back inside, 0 leaves
    two = ref.begin(1, (0, 1))
    assert ref.step(PAREN, tab, two, [1], END) == one and ref.step(PAREN, tab, two, [2], END) == (2, True, False, False, ())
    assert ref.allowed(PAREN, tab, two, END) == {0, 1, 2, 3, 4, 5}
    # depth equal to max_depth: no opener, not even one that closes again inside the token
    assert ref.allowed(PAREN, tab, one, END, max_depth=1) == {1, 4, 5} and ref.allowed(PAREN, tab, two, END, max_depth=2) == {1, 2, 4, 5}
    assert ref.step(PAREN, tab, one, [0], END, max_depth=1) == ref.BROKEN
    # END only at depth 0
    out = (2, True, False, False, ())
    assert ref.allowed(PAREN, tab, out, END) == {9} and ref.step(PAREN, tab, out, [9], END) == (2, False, False, True, ())
    assert ref.allowed(PAREN, tab, ref.begin(1), END) == {0, 3, 5, 9} and 9 not in ref.allowed(PAREN, tab, one, END)
    assert ref.settle(PAREN, tab, ref.begin(2, (1,)), END) == ref.BROKEN
    # masks and state rows
    assert ref.mask(PAREN, tab, s0, 1, END).tolist() == [0b101001] and ref.mask(PAREN, tab, one, 1, END).tolist() == [0b111011]
    assert ref.mask(PAREN, tab, out, 1, END).tolist() == [1 << 9] and ref.mask(PAREN, tab, ref.FREE, 2, END).tolist() == [0xFFFFFFFF] * 2
    assert ref.state_row(s0) == [1 << 16, 0, 0, 0, 0] and ref.state_row(two) == [1 | 1 << 16 | 2 << 24, 0x10, 0, 0, 0]
    assert ref.state_row(ref.begin(1, (1,) * 17)) == [1 | 1 << 16 | 17 << 24, 0x1111111111111111, 1, 0, 0]
    assert ref.state_row((2, False, False, True, ())) == [2 | 1 << 18, 0, 0, 0, 0] and ref.state_row(ref.BROKEN) == [1 << 17, 0, 0, 0, 0]
    assert ref.row_state(ref.raw_row(1, con=True, depth=2, nibbles=(0, 1, 7))) == two
    assert ref.load(tab, ref.begin(1, (1,) * 5), 4) == ref.BROKEN and ref.load(tab, ref.begin(3), 64) == ref.BROKEN
    # the index: "a" never touches; everything else meets ( or ) -- valid or not -- from states 0 and 1; state 2 walks nothing
    rows, some, dep = ref.index(PAREN, tab, 1)
    assert rows[:, 0].tolist() == [1 << 5, 1 << 5, 0] and some.tolist() == [1, 1, 0] and dep == [[0, 1, 2, 3, 4], [0, 1, 2, 3, 4], []]
    assert ref.touches(tab, 0, b"a)") == "touch" and ref.touches(tab, 2, b"a") == "dead" and ref.touches(tab, 1, b"a") == "free"
    # an op byte that is no op, a ret row that does not exist, a return state that is no state: DEAD
    trans, ret, op, accept = (x.copy() for x in tab)
    op[1, ord("a")] = 0x30
    assert ref.walk((trans, ret, op, accept), 1, (0,), b"a", 64) is None
    trans[1, ord(")")] = 1
    assert ref.walk((trans, ret, op, accept), 1, (0,), b")", 64) is None
    trans[1, ord(")")], ret[0, 0] = 0, 3
    assert ref.walk((trans, ret, op, accept), 1, (0,), b")", 64) is None and ref.walk(tab, 1, (0,), b")", 64) == (2, ())
    assert ref.table_bytes(tab).shape == (3 * 769 + 32,)


def test_product_nest_table_agrees_with_the_definition():
    from splintr_amd import dfa, nest
    tab = cases.brackets_table()
    t = nest.NestTable(tab[0], tab[2], tab[1], tab[3])
    assert t.table().tolist() == ref.table_bytes(tab).tolist() and (t.n_states, t.n_ret) == (2, 2)
    for data in (b"", b"a", b"(a)", b"()", b"[]", b"[a]", b"(]", b"([a]a)", b"((", b")", b"(" * 64 + b")" * 64, b"(" * 65 + b")" * 65):
        for max_depth in (2, 64):
            want = ref.walk(tab, 0, (), data, max_depth)
            assert t.walk(0, (), data, max_depth) == want
            assert t.matches(data, max_depth) == (want is not None and bool(tab[3][want[0]]) and not want[1]), data
    assert t.shortest_completion(1, (1, 2, 1)) == b")])" and t.shortest_completion(0, ()) == b"" and t.shortest_completion(1, (2,)) == b"a]"
    d = dfa.compile_regex(rb"(ab|c)*a{1,3}")
    z = nest.from_dfa(d)
    assert z.n_ret == 0 and not z.op.any() and z.table().shape == (d.n_states * 769,)
    for data in (b"", b"a", b"abca", b"caaa", b"aaaa", b"b"):
        assert z.matches(data) == d.matches(data)


# ---------------------------------------------------------------------------------------------- the anchor: every op zero
@pytest.mark.parametrize("name", sorted(dfa_cases.TOYS))
@pytest.mark.parametrize("lanes, ilanes, s_block", SHAPES)
def test_sim_anchor_index(sim, name, lanes, ilanes, s_block):
    _, index = runners(sim, name, lanes, ilanes, s_block)
    dfa_cases.check_index(cases.dfa_index(index), name, extra_words=(0, 1, 3))


@pytest.mark.parametrize("name", sorted(dfa_cases.TOYS))
def test_sim_anchor_against_guided_choice_and_every_probe_id(sim, name):
    lanes = SHAPES[sorted(dfa_cases.TOYS).index(name) % len(SHAPES)][0]
    run = cases.dfa_run(runners(sim, name, lanes)[0])
    dfa_cases.check_against_choice(run, name, steps=6)
    dfa_cases.check_every_probe_id_from_every_state(run, name)


@pytest.mark.parametrize("lanes, ilanes, s_block", SHAPES)
def test_sim_anchor_end_ids_flags_layout_and_load(sim, lanes, ilanes, s_block):
    run, index = runners(sim, "gaps", lanes, ilanes, s_block)
    dfa_cases.check_end_ids(cases.dfa_run(run))
    dfa_cases.check_flags(cases.dfa_run(run))
    dfa_cases.check_layout_and_load(cases.dfa_run(run), cases.dfa_index(index))
    run, index = runners(sim, "gaps", lanes, ilanes, s_block, v4=False)             # word accesses where 16-byte accesses would do
    dfa_cases.check_layout_and_load(cases.dfa_run(run), cases.dfa_index(index))


# ---------------------------------------------------------------------------------------------- tables with ops
@pytest.mark.parametrize("name", ["brackets", "gaps", "edges"])
@pytest.mark.parametrize("lanes, ilanes, s_block", SHAPES)
def test_sim_index_of_random_tables(sim, name, lanes, ilanes, s_block):
    _, index = runners(sim, name, lanes, ilanes, s_block)
    cases.check_index(index, name, extra_words=(0, 1, 3))


def test_sim_index_4096_states(sim):
    _, index = runners(sim, "brackets")
    cases.check_index(index, "brackets", sizes=(4096,))


@pytest.mark.parametrize("lanes, ilanes, s_block", SHAPES)
def test_sim_dep_lists_and_dep_cap(sim, lanes, ilanes, s_block):
    run, index = runners(sim, "deps", lanes, ilanes, s_block)
    assert cases.check_deps(index, run) == sum(cases.DEP_LENGTHS) + 256


@pytest.mark.parametrize("lanes, ilanes, s_block", SHAPES)
def test_sim_stack_state_row_end_flags_and_layouts(sim, lanes, ilanes, s_block):
    run, index = runners(sim, "brackets", lanes, ilanes, s_block)
    cases.check_stack(run)
    cases.check_flags_and_layouts(run, index)
    cases.check_end_depth(runners(sim, "paren", lanes)[0])
    run, index = runners(sim, "brackets", lanes, ilanes, s_block, v4=False)
    cases.check_flags_and_layouts(run, index)


def test_sim_mutant_pop_fails_the_stack_check(sim):
    cases.check_stack(runners(sim, "brackets")[0])
    with pytest.raises(AssertionError):
        cases.check_stack(runners(sim, "brackets", mutant="pop")[0])


def test_sim_mutant_end_fails_the_end_depth_check(sim):
    cases.check_end_depth(runners(sim, "paren")[0])
    with pytest.raises(AssertionError):
        cases.check_end_depth(runners(sim, "paren", mutant="end")[0])


def test_sim_mutant_dep_fails_the_deps_check(sim):
    with pytest.raises(AssertionError):
        cases.check_deps(*reversed(runners(sim, "deps", mutant="dep")))


def test_sim_geometry_matches_the_reference(sim):
    g = sim.geometry()
    assert (g["max_depth"], g["state_words"], g["max_ret"], g["push"], g["pop"]) == (ref.MAX_DEPTH, ref.STATE_WORDS, ref.MAX_RET, ref.PUSH, ref.POP)
    assert (g["max_states"], g["max_end"]) == (dfa_ref.MAX_STATES, dfa_ref.MAX_END) and g["piece"] % 4 == 0


# ---------------------------------------------------------------------------------------------- the C ABI's refusals (no device is touched)
@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as entry
    entry.build()
    from splintr_amd import _ffi
    return _ffi


def test_abi_refuses_before_the_device(ffi):
    L = ffi.lib()
    i, o, out = ffi.SplNestIn(1, 1), ffi.SplNestOpts(0, 4, (7,), 8), ffi.SplNestOut()
    assert L.spl_nest_step_device(None, ctypes.byref(i), ctypes.byref(o), ctypes.byref(out), None) == SPL_EINVAL
    assert b"spl_nest_step_device: null handle" in L.spl_last_error()
    n = ctypes.c_uint32(0)
    assert L.spl_nest_index_device(None, None, 1, 0, 1, None, 0, ctypes.byref(n), None) == SPL_EINVAL and b"spl_nest_index_device: null handle" in L.spl_last_error()
    assert L.spl_nest_reserve_device(None) == SPL_EINVAL and b"spl_nest_reserve_device: null handle" in L.spl_last_error()
    assert ctypes.sizeof(ffi.SplNestOpts) == 56 and ctypes.sizeof(ffi.SplNestIn) == 80 and ctypes.sizeof(ffi.SplNestOut) == 32
    assert (ffi.SPL_NEST_KEEP_FREE, ffi.SPL_NEST_I64) == (ref.KEEP_FREE, ref.I64) == (2, 4)
    hdr = open(ffi.__file__.replace("splintr_amd/_ffi.py", "include/splintr_hip.h")).read()
    for name, val in (("SPL_NEST_PUSH", "0x10"), ("SPL_NEST_POP", "0x20"), ("SPL_NEST_MAX_STATES", "4096"), ("SPL_NEST_MAX_RET", "4096"),
                      ("SPL_NEST_MAX_DEPTH", "64"), ("SPL_NEST_STATE_WORDS", "5"), ("SPL_NEST_MAX_END", "8")):
        assert "#define %s %s%s" % (name, " " * (20 - len(name)), val) in hdr, name
        assert getattr(ffi, name) == eval(val)
    assert (ffi.SPL_NEST_MAX_DEPTH, ffi.SPL_NEST_STATE_WORDS, ffi.SPL_NEST_MAX_RET, ffi.SPL_NEST_PUSH, ffi.SPL_NEST_POP) == \
        (ref.MAX_DEPTH, ref.STATE_WORDS, ref.MAX_RET, ref.PUSH, ref.POP)
    assert "#define SPL_NEST_TABLE_BYTES(n_states, n_ret) ((size_t)(n_states) * 769 + (size_t)(n_ret) * 32)" in hdr
    assert "((size_t)(n_states) * ((((size_t)(n_words) + 3) & ~(size_t)3) * 4 + 5) + 4 + (size_t)(dep_cap) * 4)" in hdr
    assert ffi.SPL_NEST_TABLE_BYTES(3, 2) == 3 * 769 + 64 and ffi.SPL_NEST_INDEX_BYTES(3, 5, 7) == 3 * 32 + 16 + 28 + 3
    assert ffi.SPL_NEST_INDEX_BYTES(2, 8, 0) == ffi.SPL_DFA_INDEX_BYTES(2, 8) + 12
