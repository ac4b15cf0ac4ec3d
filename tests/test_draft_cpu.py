"""Draft verification without a GPU: the definition (tests/draft_ref.py) pinned by a hand-worked tree, and the code the kernels run
(splintr_amd/csrc/spl_k_draft.h, evaluated by tests/hostsim/draft_sim.cpp with 64, 5, 3 and 1 lanes) against that definition through the
checks of tests/draft_cases.py -- the anchor against the STEP's own simulation, topologies, orphans, lengths, ids, input states, the nest
guide's stack and dependent ids, flags and layouts -- plus three mutants of the header that a named check must catch, and the C ABI's
refusals that need no device."""
import ctypes

import numpy as np
import pytest

import draft_cases as cases
import draft_ref as ref
import nest_cases
import nest_ref

LANES = (64, 5, 3, 1)
SPL_EINVAL = -1


@pytest.fixture(scope="module")
def sim():
    import draft_sim
    draft_sim.lib()
    return draft_sim


_vocabs = {}


def _v(sim, name):
    if name not in _vocabs:
        vocab, specials, _ = cases.vocab(name)
        _vocabs[name] = sim.Vocab(vocab, specials)
    return _vocabs[name]


def drafter(sim, name, lanes=64, mutant="", v4=None):
    v = _v(sim, name)

    def draft(kind, table, n_states, n_ret, **kw):
        return sim.draft(v, kind, table, n_states, n_ret, lanes=lanes, mutant=mutant, v4=v4, **kw)
    return draft


def stepper(sim, name, lanes=64):
    """the STEP's simulations (tests/hostsim/dfa_sim.py, nest_sim.py) over the same vocabulary object"""
    import dfa_sim
    import nest_sim as ns
    v = _v(sim, name)

    def step(kind, table, n_states, n_ret, *, max_depth=64, **kw):
        if kind == "dfa":
            return dfa_sim.run(v, table, n_states, lanes=lanes, **kw)
        return ns.run(v, table, n_states, n_ret, max_depth=max_depth, lanes=lanes, **kw)
    return step


# ---------------------------------------------------------------------------------------------- the definition, by hand
PAREN = nest_ref.ordinary(nest_cases.vocab_paren()[0])              # 0 "("  1 ")"  2 "))"  3 "()"  4 "a)"  5 "a"
END = (9,)


def test_ref_tree_by_hand():
    """The three-state a* ( ... ) table.  From (0, empty):

        node 0  "("   below the root     -> (1, (0,))                      ok
        node 1  "a)"  below node 0       -> pops symbol 0: (2, ())         ok    -- state 2 accepts, the stack is empty
        node 2  END   below node 1       -> done in state 2                ok    -- an END id in mid-path ...
        node 3  "a"   below node 2       -> not read: the done row         NOT ok -- ... with a child under it
        node 4  ")"   below the root     -> nothing to pop: broken         NOT ok -- a rejected id ...
        node 5  "a"   below node 4       -> not read: the broken row       NOT ok -- ... with a child
    (six nodes: the five of the tree and the rejected id's child)"""
    tab = nest_cases.paren_table()
    ids, parent = [0, 4, 9, 5, 1, 5], [-1, 0, 1, 2, -1, 4]
    assert [ref.kind_of(parent, i, 6) for i in range(6)] == ["node"] * 6
    assert ref.path(parent, 3) == [0, 1, 2, 3] and ref.path(parent, 5) == [4, 5] and ref.path(None, 2) == [0, 1, 2]
    rows, ok = ref.draft("nest", PAREN, tab, nest_ref.begin(0), ids, parent, 1, END)
    assert ok == [1, 1, 1, 0, 0, 0]
    done, ones = (2, False, False, True, ()), [0xFFFFFFFF]
    assert [s for s, _ in rows] == [nest_ref.begin(0), (1, True, False, False, (0,)), (2, True, False, False, ()), done, done, nest_ref.BROKEN, nest_ref.BROKEN]
    assert [m.tolist() for _, m in rows] == [[0b101001], [0b111011], [1 << 9], ones, ones, ones, ones]
    # the same ids as a chain: "(" | "a)" | END | then nothing is read
    rows, ok = ref.draft("nest", PAREN, tab, nest_ref.begin(0), ids, None, 1, END)
    assert ok == [1, 1, 1, 0, 0, 0] and [s for s, _ in rows][3:] == [done] * 4
    # absent nodes and orphans
    assert [ref.kind_of(parent, i, 3) for i in range(6)] == ["node", "node", "node", "absent", "absent", "absent"]
    assert [ref.kind_of([-1, 0, 2, 2, 5, -2], i, 6) for i in range(6)] == ["node", "node", "orphan", "orphan", "orphan", "orphan"]
    assert [ref.kind_of([-1, 0, 1, -1, 1], i, 2) for i in range(5)] == ["node", "node", "absent", "absent", "absent"]
    assert ref.kind_of([-1, 3, 1, -1], 2, 4) == "orphan" and ref.kind_of([-1, -1, 1, 2], 3, 3) == "absent" and ref.kind_of([-1, 5], 1, 1) == "absent"
    rows, ok = ref.draft("nest", PAREN, tab, nest_ref.begin(0), [0, 5, 5, 5], [-1, 0, 2, 2], 1, END, length=3)
    assert ok == [1, 1, 0, 0] and rows[3][0] == rows[4][0] == nest_ref.BROKEN and rows[3][1].tolist() == ones
    # a sequence that is free on input: nothing is read, everything is acceptable; done and broken on input: nothing is
    assert ref.draft("nest", PAREN, tab, nest_ref.FREE, [1, 1], None, 1, END)[1] == [1, 1]
    assert ref.draft("nest", PAREN, tab, done, [5], None, 1, END)[1] == [0] and ref.draft("nest", PAREN, tab, nest_ref.BROKEN, [5], None, 1, END)[1] == [0]
    assert ref.clamp(-1, 4) == 0 and ref.clamp(9, 4) == 4 and ref.clamp(None, 4) == 4


def test_sim_runs_the_hand_worked_tree(sim):
    tab = nest_cases.paren_table()
    for lanes in LANES:
        r, wants = cases.expect(drafter(sim, "paren", lanes), "nest", PAREN, tab, nest_cases.rows_of([nest_ref.begin(0)]), [nest_ref.begin(0)],
                                [[0, 4, 9, 5, 1, 5]], [-1, 0, 1, 2, -1, 4], 1, END)
        assert r["ok"].tolist() == [[1, 1, 1, 0, 0, 0]] and r["live"].tolist() == [[1, 1, 1, 0, 0, 0, 0]]


# ---------------------------------------------------------------------------------------------- the checks
@pytest.mark.parametrize("name", sorted(cases.dfa_cases.TOYS))
def test_sim_anchor_against_the_step(sim, name):
    lanes = LANES[sorted(cases.dfa_cases.TOYS).index(name) % len(LANES)]
    cases.check_anchor(drafter(sim, name, lanes), stepper(sim, name, lanes), name)


def test_sim_anchor_with_a_stack(sim):
    cases.check_anchor(drafter(sim, "brackets"), stepper(sim, "brackets"), "brackets", kinds=("nest",))


@pytest.mark.parametrize("lanes", LANES)
def test_sim_topologies(sim, lanes):
    cases.check_topologies(drafter(sim, "gaps", lanes), "gaps", kinds=("dfa",))
    cases.check_topologies(drafter(sim, "brackets", lanes), "brackets", kinds=("nest",))


@pytest.mark.parametrize("name", ["chain", "edges"])                 # ("long": 128-byte tokens make the brute-force definition take minutes)
def test_sim_topologies_of_other_toy_vocabularies(sim, name):
    cases.check_topologies(drafter(sim, name), name, row_lens=(2, 63))


@pytest.mark.parametrize("lanes", LANES)
def test_sim_orphans_lengths_ids_and_input_states(sim, lanes):
    d, b = drafter(sim, "gaps", lanes), drafter(sim, "brackets", lanes)
    cases.check_orphans(d)
    cases.check_orphans(b, "brackets", "nest")
    cases.check_lengths(d)
    cases.check_lengths(b, "brackets", "nest")
    cases.check_order(d)
    cases.check_order(b, "brackets", "nest")
    cases.check_rejected(d)
    cases.check_rejected(b, "brackets", "nest")
    cases.check_done_child(d)
    cases.check_done_child(b, "brackets", "nest")

    def both(kind, *a, **kw):
        return (d if kind == "dfa" else b)(kind, *a, **kw)
    cases.check_input_states(both)


@pytest.mark.parametrize("lanes", LANES)
def test_sim_stack_and_dependent_ids(sim, lanes):
    cases.check_stack(drafter(sim, "brackets", lanes))
    cases.check_deps(drafter(sim, "deps", lanes))


@pytest.mark.parametrize("lanes", LANES)
def test_sim_layouts_and_flags(sim, lanes):
    def both(v4):
        d, b = drafter(sim, "gaps", lanes, v4=v4), drafter(sim, "brackets", lanes, v4=v4)
        return lambda kind, *a, **kw: (d if kind == "dfa" else b)(kind, *a, **kw)
    cases.check_layout_and_flags(both(None))
    cases.check_layout_and_flags(both(False))                         # word accesses where 16-byte accesses would do: a base off its alignment


# ---------------------------------------------------------------------------------------------- mutants
def test_sim_mutant_order_fails_the_order_check_alone(sim):
    for name, kind in (("gaps", "dfa"), ("brackets", "nest")):
        m = drafter(sim, name, mutant="order")
        with pytest.raises(AssertionError):
            cases.check_order(m, name, kind)
    # paths of one id have no order: the checks over stars and single nodes do not notice
    cases.check_lengths(drafter(sim, "gaps", mutant="order"), chains=False)
    cases.check_topologies(drafter(sim, "gaps", mutant="order"), "gaps", kinds=("dfa",), row_lens=(0, 1))


def test_sim_mutant_ok_fails_the_rejected_check_alone(sim):
    for name, kind in (("gaps", "dfa"), ("brackets", "nest")):
        m = drafter(sim, name, mutant="ok")
        with pytest.raises(AssertionError):
            cases.check_rejected(m, name, kind)
        cases.check_order(m, name, kind)
        cases.check_done_child(m, name, kind)


def test_sim_mutant_done_fails_the_done_child_check_alone(sim):
    for name, kind in (("gaps", "dfa"), ("brackets", "nest")):
        m = drafter(sim, name, mutant="done")
        with pytest.raises(AssertionError):
            cases.check_done_child(m, name, kind)
        cases.check_order(m, name, kind)
        cases.check_rejected(m, name, kind)


def test_sim_geometry_matches_the_reference(sim):
    assert sim.geometry() == dict(max_nodes=ref.MAX_NODES, parent_per_seq=ref.PARENT_PER_SEQ)


# ---------------------------------------------------------------------------------------------- the C ABI's refusals (no device is touched)
@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as entry
    entry.build()
    from splintr_amd import _ffi
    return _ffi


def test_abi_refuses_before_the_device(ffi):
    L = ffi.lib()
    d = ffi.SplDraftOut()
    i, o = ffi.SplDfaIn(1, 1), ffi.SplDfaOpts(0, 4, (7,))
    assert L.spl_dfa_draft_device(None, ctypes.byref(i), ctypes.byref(o), ctypes.byref(d), None) == SPL_EINVAL
    assert b"spl_dfa_draft_device: null handle" in L.spl_last_error()
    i, o = ffi.SplNestIn(1, 1), ffi.SplNestOpts(0, 4, (7,), 8)
    assert L.spl_nest_draft_device(None, ctypes.byref(i), ctypes.byref(o), ctypes.byref(d), None) == SPL_EINVAL
    assert b"spl_nest_draft_device: null handle" in L.spl_last_error()
    assert ctypes.sizeof(ffi.SplDraftOut) == 48
    assert (ffi.SPL_DRAFT_MAX_NODES, ffi.SPL_DRAFT_PARENT_PER_SEQ) == (ref.MAX_NODES, ref.PARENT_PER_SEQ) == (64, 1)
    hdr = open(ffi.__file__.replace("splintr_amd/_ffi.py", "include/splintr_hip.h")).read()
    assert "#define SPL_DRAFT_MAX_NODES      64" in hdr and "#define SPL_DRAFT_PARENT_PER_SEQ 1u" in hdr
    assert "spl_dfa_draft_device" in ffi.SYMBOLS and "spl_nest_draft_device" in ffi.SYMBOLS


def test_python_layer_refuses_without_a_device():
    import torch
    from splintr_amd import device as dv
    ids = torch.zeros((2, 65), dtype=torch.int32)
    with pytest.raises(ValueError, match="at most 64 nodes"):
        dv.check_draft_args(ids, None)
    with pytest.raises(ValueError, match="rank 2"):
        dv.check_draft_args(ids[0], None)
    ids = torch.zeros((2, 3), dtype=torch.int32)
    for bad in (torch.zeros(3, dtype=torch.int64), torch.zeros(4, dtype=torch.int32), torch.zeros((3, 3), dtype=torch.int32), [-1, 0, 1]):
        with pytest.raises(ValueError, match="parent must be"):
            dv.check_draft_args(ids, bad)
    dv.check_draft_args(ids, torch.tensor([-1, 0, 1], dtype=torch.int32))
    dv.check_draft_args(ids, torch.zeros((2, 3), dtype=torch.int32))
    with pytest.raises(ValueError, match="keep_free needs"):
        dv.check_draft_args(ids, None, keep_free=True)
    with pytest.raises(ValueError, match=r"\[batch, 1 \+ nodes, n_words\]"):
        dv.check_draft_args(ids, None, mask=torch.zeros((2, 3, 4), dtype=torch.int32), n_words=4)
    r = dv.DraftResult(torch.zeros((2, 4, 4), dtype=torch.int32), torch.tensor([[1, 1, 0], [1, 0, 0]], dtype=torch.uint8), None, None, tree=False)
    assert r.accepted_len().tolist() == [2, 1]
    with pytest.raises(ValueError, match="a chain's"):
        dv.DraftResult(r.mask, r.ok, None, None, tree=True).accepted_len()
