"""GPU tests (-m gpu): spl_nest_index_device and spl_nest_step_device -- JSON mode, allowed-token bitmasks from a byte automaton with a stack
-- through the C ABI into guarded buffers against the definition of tests/nest_ref.py: the checks of tests/nest_cases.py (the ops-zero
anchor over the toy vocabularies of tests/dfa_cases.py included), batch sizes around the kernels' edges, a mask base and an index base off
their 16-byte alignment, the refusals, the shipped vocabularies end to end with json_guide against a numpy brute force, a uniform sampler
and Python's own JSON parser, NestGuide beside the streaming decode, and an ops-zero table beside RegexGuide."""
import ctypes
import json
import random

import numpy as np
import pytest

import dfa_cases
import nest_cases as cases
import nest_ref as ref
import vocabgen

pytestmark = pytest.mark.gpu

WORD_POISON = 0x5A5A5A5A5A5A5A5A
MASK_POISON = 0x5A5A5A5A
PATTERN = r"[a-z]+|\s+|[^a-z\s]+"
SPL_ECAPACITY = -3

_toks = {}


def _toy(name, tmp_path_factory):
    if name not in _toks:
        from splintr_amd import Tokenizer
        vocab, specials, _ = cases.vocab(name)
        path = tmp_path_factory.mktemp("nest") / (name + ".tiktoken")
        path.write_bytes(vocabgen.tiktoken({b: i for i, b in vocab.items()}))
        _toks[name] = Tokenizer(str(path), PATTERN, {v.decode(): k for k, v in specials.items()})
    return _toks[name]


def _index(tok, table, n_states, n_ret, n_words, dep_cap=None, *, off=0, keep=False):
    """spl_nest_index_device into a poisoned buffer `off` bytes (a multiple of 4) behind a 16-byte boundary -> (rows uint32 [S, stride],
    some uint8 [S], dep_off uint32 [S + 1], dep_ids uint32 [dep_cap]); asserts that nothing around the index was written.  dep_cap None:
    the exact size, found by a first build with dep_cap 0.  A refused build raises cases.TooSmall(n_dep) after checking that no dependent
    entry and nothing behind the index was written.  keep: also the device tensors (table, index view) and dep_cap."""
    import torch
    from splintr_amd import _ffi
    if dep_cap is None:
        try:
            return _index(tok, table, n_states, n_ret, n_words, 0, off=off, keep=keep)
        except cases.TooSmall as e:
            dep_cap = e.args[0]
    dev = torch.device("cuda", 0)
    stride = ref.stride(n_words)
    size = _ffi.SPL_NEST_INDEX_BYTES(n_states, n_words, dep_cap)
    assert size == n_states * stride * 4 + 4 * (n_states + 1) + 4 * dep_cap + n_states
    flat = torch.full((off + size + 64,), 0x5A, dtype=torch.uint8, device=dev)
    view = flat[off:off + size]
    assert view.data_ptr() % 16 == off % 16
    t_tab = torch.from_numpy(np.ascontiguousarray(table, dtype=np.uint8)).to(dev)
    n_dep = ctypes.c_uint32(0xFFFFFFFF)
    rc = _ffi.lib().spl_nest_index_device(tok.handle, t_tab.data_ptr(), n_states, n_ret, n_words, view.data_ptr(), dep_cap, ctypes.byref(n_dep),
                                          torch.cuda.current_stream(dev).cuda_stream)
    whole = flat.cpu().numpy()
    assert (whole[:off] == 0x5A).all() and (whole[off + size:] == 0x5A).all(), "written around the index"
    a = off + n_states * stride * 4
    b = a + 4 * (n_states + 1)
    c = b + 4 * dep_cap
    if rc == SPL_ECAPACITY:
        assert b"dep_cap is too small" in _ffi.lib().spl_last_error() and n_dep.value > dep_cap
        assert (whole[b:c] == 0x5A).all(), "a refused build wrote dependent entries"
        raise cases.TooSmall(int(n_dep.value))
    assert rc == 0, _ffi.last_error()
    rows = whole[off:a].copy().view(np.uint32).reshape(n_states, stride)
    dep_off = whole[a:b].copy().view(np.uint32)
    dep_ids = whole[b:c].copy().view(np.uint32)
    some = whole[c:c + n_states].copy()
    assert int(dep_off[n_states]) == n_dep.value <= dep_cap and (dep_ids[n_dep.value:] == MASK_POISON).all(), "entries behind n_dep were written"
    return (rows, some, dep_off, dep_ids, t_tab, view, dep_cap) if keep else (rows, some, dep_off, dep_ids)


def _call(tok, table, n_states, n_ret, *, ids, state, max_depth=64, lengths=None, flags=0, end_ids=(), n_words, in_place=False, mask_init=None,
          want_live=True, off16=0, index_off=0):
    """One step through the C ABI (the index built by the kernels in front of it) with poisoned outputs and a spare row behind each -> dict
    of numpy arrays; asserts that nothing behind the rows was written and that KEEP_FREE left the rows of sequences that are not
    constrained alone.  off16: words the mask base lies behind a 16-byte boundary; index_off: bytes the index lies behind one."""
    import torch
    from splintr_amd import _ffi
    dev = torch.device("cuda", 0)
    ids = np.ascontiguousarray(ids)
    B, K = ids.shape
    if ids.dtype == np.int64:
        flags |= ref.I64
    _, _, _, _, t_tab, t_index, dep_cap = _index(tok, table, n_states, n_ret, n_words, off=index_off, keep=True)
    t_ids = torch.from_numpy(ids.view(np.int32) if ids.dtype == np.uint32 else ids).to(dev)
    t_len = None if lengths is None else torch.from_numpy(np.ascontiguousarray(lengths, dtype=np.int32)).to(dev)
    rows = np.concatenate([np.asarray(state, dtype=np.uint64).reshape(B, ref.STATE_WORDS), np.full((1, ref.STATE_WORDS), WORD_POISON, dtype=np.uint64)])
    t_sin = torch.from_numpy(rows.view(np.int64)).to(dev)
    t_sout = t_sin if in_place else torch.full((B + 1, ref.STATE_WORDS), WORD_POISON, dtype=torch.int64, device=dev)
    flat = torch.full(((B + 1) * n_words + 4,), MASK_POISON, dtype=torch.int32, device=dev)
    t_mask = flat[off16:off16 + (B + 1) * n_words].view(B + 1, n_words)
    assert t_mask.data_ptr() % 16 == 4 * off16
    init = None
    if mask_init is not None:
        init = np.asarray(mask_init, dtype=np.uint32)
        t_mask[:B] = torch.from_numpy(init.view(np.int32)).to(dev)
    t_live = torch.full((B + 1,), 0x5A, dtype=torch.uint8, device=dev)
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    si = _ffi.SplNestIn(B, K, ptr(t_ids), ptr(t_len), t_sin.data_ptr(), t_tab.data_ptr(), t_index.data_ptr(), n_states, n_ret, dep_cap, t_index.numel())
    o = _ffi.SplNestOpts(flags, n_words, end_ids, max_depth)
    so = _ffi.SplNestOut(t_sout.data_ptr(), t_mask.data_ptr(), t_live.data_ptr() if want_live else None)
    rc = _ffi.lib().spl_nest_step_device(tok.handle, ctypes.byref(si), ctypes.byref(o), ctypes.byref(so), torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, _ffi.last_error()
    st = t_sout.cpu().numpy().view(np.uint64)
    whole = flat.cpu().numpy().view(np.uint32)
    mask = whole[off16:off16 + (B + 1) * n_words].reshape(B + 1, n_words)
    live = t_live.cpu().numpy()
    assert (st[B] == WORD_POISON).all() and (mask[B] == MASK_POISON).all() and live[B] == 0x5A, "written behind the rows"
    assert (whole[:off16] == MASK_POISON).all() and (whole[off16 + (B + 1) * n_words:] == MASK_POISON).all(), "written around the mask"
    if not want_live:
        assert (live == 0x5A).all()
    elif flags & ref.KEEP_FREE:
        keep = live[:B] == 0
        assert (mask[:B][keep] == (init[keep] if init is not None else MASK_POISON)).all(), "KEEP_FREE: a row that is not constrained was written"
    return dict(state=st[:B].copy(), mask=mask[:B].copy(), live=live[:B].copy())


def _runner(tok, **fixed):
    return lambda table, n_states, n_ret, **kw: _call(tok, table, n_states, n_ret, **dict(fixed, **kw))


def _indexer(tok, **fixed):
    return lambda table, n_states, n_ret, n_words, dep_cap=None: _index(tok, table, n_states, n_ret, n_words, dep_cap, **fixed)


# ---------------------------------------------------------------------------------------------- the anchor: every op zero
@pytest.mark.parametrize("name", sorted(dfa_cases.TOYS))
def test_anchor_index(name, tmp_path_factory):
    tok = _toy(name, tmp_path_factory)
    dfa_cases.check_index(cases.dfa_index(_indexer(tok)), name, extra_words=(0, 1, 3))
    dfa_cases.check_index(cases.dfa_index(_indexer(tok, off=4)), name, sizes=(2, 65))


def test_anchor_index_4096_states(tmp_path_factory):
    dfa_cases.check_index(cases.dfa_index(_indexer(_toy("gaps", tmp_path_factory))), "gaps", sizes=(4096,))


@pytest.mark.parametrize("name", sorted(dfa_cases.TOYS))
def test_anchor_against_guided_choice_and_every_probe_id(name, tmp_path_factory):
    run = cases.dfa_run(_runner(_toy(name, tmp_path_factory)))
    dfa_cases.check_against_choice(run, name, steps=6)
    dfa_cases.check_every_probe_id_from_every_state(run, name)


def test_anchor_end_flags_layout_and_load(tmp_path_factory):
    tok = _toy("gaps", tmp_path_factory)
    run, index = cases.dfa_run(_runner(tok)), cases.dfa_index(_indexer(tok))
    dfa_cases.check_end_ids(run)
    dfa_cases.check_flags(run)
    dfa_cases.check_layout_and_load(run, index)
    # a mask base 4 bytes behind a 16-byte boundary, an index base 8 bytes behind one: word accesses, whatever the row width
    dfa_cases.check_layout_and_load(cases.dfa_run(_runner(tok, off16=1)), index)
    dfa_cases.check_layout_and_load(cases.dfa_run(_runner(tok, index_off=8)), cases.dfa_index(_indexer(tok, off=8)))
    dfa_cases.check_end_ids(cases.dfa_run(_runner(tok, off16=3)))


# ---------------------------------------------------------------------------------------------- tables with ops
@pytest.mark.parametrize("name", ["brackets", "gaps", "edges"])
def test_index_of_random_tables(name, tmp_path_factory):
    tok = _toy(name, tmp_path_factory)
    cases.check_index(_indexer(tok), name, extra_words=(0, 1, 3))
    cases.check_index(_indexer(tok, off=4), name, sizes=(2, 65))


def test_index_4096_states(tmp_path_factory):
    cases.check_index(_indexer(_toy("brackets", tmp_path_factory)), "brackets", sizes=(4096,))


def test_dep_lists_and_dep_cap(tmp_path_factory):
    tok = _toy("deps", tmp_path_factory)
    assert cases.check_deps(_indexer(tok), _runner(tok)) == sum(cases.DEP_LENGTHS) + 256
    cases.check_deps(_indexer(tok, off=12), _runner(tok, off16=1, index_off=12))


def test_stack_state_row_end_flags_and_layouts(tmp_path_factory):
    tok = _toy("brackets", tmp_path_factory)
    cases.check_stack(_runner(tok))
    cases.check_flags_and_layouts(_runner(tok), _indexer(tok))
    cases.check_flags_and_layouts(_runner(tok, off16=1), _indexer(tok))
    cases.check_flags_and_layouts(_runner(tok, index_off=8, want_live=True), _indexer(tok, off=8))
    cases.check_end_depth(_runner(_toy("paren", tmp_path_factory)))
    cases.check_end_depth(_runner(_toy("paren", tmp_path_factory), off16=3))


@pytest.mark.parametrize("B", [0, 1, 63, 64, 65, 1025])
def test_batch_sizes(B, tmp_path_factory):
    tok = _toy("brackets", tmp_path_factory)
    vocab, specials, toks = cases.vocab("brackets")
    nw = cases.min_words(vocab)
    tab = cases.brackets_table()
    rng = random.Random(B)
    stacks = [(), (1,), (2, 1), (1,) * 16, (2,) * 17, (1, 2) * 32]
    start = [ref.begin(rng.randrange(2), rng.choice(stacks)) if b % 7 else ref.FREE for b in range(B)]
    ids = [[rng.choice(sorted(vocab))] for _ in range(B)]
    r, _ = cases.expect(_runner(tok), toks, tab, cases.rows_of(start), start, np.array(ids, dtype=np.int32).reshape(B, 1), nw, (25, 63))
    assert r["state"].shape == (B, 5)


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals(tmp_path_factory):
    import torch
    from splintr_amd import _ffi, device as dv, nest
    tok = _toy("brackets", tmp_path_factory)
    vocab, specials, _ = cases.vocab("brackets")
    L = _ffi.lib()
    dev = torch.device("cuda", 0)
    nw = cases.min_words(vocab)
    tb = cases.brackets_table()
    t = nest.NestTable(tb[0], tb[2], tb[1], tb[3])
    S, R = t.n_states, t.n_ret
    ids = torch.zeros((2, 2), dtype=torch.int32, device=dev)
    lens = torch.ones(2, dtype=torch.int32, device=dev)
    st = torch.zeros((4, 5), dtype=torch.int64, device=dev)
    st2 = torch.zeros((4, 5), dtype=torch.int64, device=dev)
    mask = torch.zeros((2, nw), dtype=torch.int32, device=dev)
    live = torch.zeros(16, dtype=torch.uint8, device=dev)
    tab = dv.nest_table(t, dev)
    index, n_dep = dv.nest_index_device(tok, tab, S, R, n_words=nw, dep_cap=1)      # (one entry is too few: built again with the exact size)
    want = ref.index(ref.ordinary(vocab), tb, nw)
    assert n_dep == sum(map(len, want[2])) > 1 and tab.shape == (S * 769 + R * 32,) and index.shape == (_ffi.SPL_NEST_INDEX_BYTES(S, nw, n_dep),)
    rows, dep_off, dep_ids, some = dv.nest_index_views(index, S, nw, n_dep)
    assert (rows.cpu().numpy().view(np.uint32) == want[0]).all() and some.cpu().tolist() == want[1].tolist()
    assert cases.dep_lists(dep_off.cpu().numpy(), dep_ids.cpu().numpy()) == want[2]
    big, n2 = dv.nest_index_device(tok, tab, S, R, n_words=nw, dep_cap=n_dep + 9)   # (built larger: cut to the entries in use)
    assert n2 == n_dep and torch.equal(big, index)

    def go(si, o, so, word):
        assert L.spl_nest_step_device(tok.handle, ctypes.byref(si) if si else None, ctypes.byref(o) if o else None, ctypes.byref(so) if so else None,
                                      None) == -1, word
        assert word in _ffi.last_error(), (word, _ffi.last_error())

    I = lambda **kw: _ffi.SplNestIn(2, 2, kw.get("ids", ids.data_ptr()), kw.get("lens", lens.data_ptr()), kw.get("state", st.data_ptr()),
                                    kw.get("table", tab.data_ptr()), kw.get("index", index.data_ptr()), kw.get("n_states", S), kw.get("n_ret", R),
                                    kw.get("dep_cap", n_dep), kw.get("index_bytes", index.numel()))
    P = lambda flags=0, n_words=nw, end=(25,), max_depth=8: _ffi.SplNestOpts(flags, n_words, end, max_depth)
    O = lambda **kw: _ffi.SplNestOut(kw.get("state", st2.data_ptr()), kw.get("mask", mask.data_ptr()), kw.get("live", live.data_ptr()))
    go(None, P(), O(), "the input struct is null")
    go(I(), None, O(), "the options are null")
    go(I(), P(), None, "the output struct is null")
    go(I(table=None), P(), O(), "d_table is null")
    go(I(index=None), P(), O(), "d_index is null")
    go(I(state=None), P(), O(), "d_state_in is null")
    go(I(), P(), O(state=None), "d_state_out is null")
    go(I(), P(), O(mask=None), "d_mask is null")
    go(I(ids=None), P(), O(), "d_ids is null")
    go(I(n_states=0), P(), O(), "n_states is 0")
    go(I(n_states=4097), P(), O(), "n_states is 4097")
    go(I(n_ret=4097), P(), O(), "n_ret is 4097")
    go(I(), P(max_depth=0), O(), "max_depth is 0")
    go(I(), P(max_depth=65), O(), "max_depth is 65")
    go(I(dep_cap=n_dep + 1), P(), O(), "the index is too small for dep_cap")
    go(I(index_bytes=index.numel() - 1), P(), O(), "the index is too small for dep_cap")
    go(I(), P(n_words=nw - 1), O(), "n_words is too small")
    go(I(), P(n_words=(1 << 26) + 1), O(), "n_words is above 2^26")
    go(I(), P(1), O(), "unknown flag bit")
    go(I(), P(8), O(), "unknown flag bit")
    go(I(), P(1 << 31), O(), "unknown flag bit")
    o = P()
    o.n_end = 9
    go(I(), o, O(), "n_end is above SPL_NEST_MAX_END")
    go(I(), P(end=()), O(), "n_end is 0")
    go(I(), P(end=(3, 32 * nw)), O(), "at or above 32 * n_words")
    go(I(), P(), O(mask=ids.data_ptr()), "coincides with an input")
    go(I(), P(), O(live=tab.data_ptr()), "coincides with an input")
    go(I(), P(), O(mask=index.data_ptr()), "coincides with an input")
    go(I(), P(), O(mask=st.data_ptr()), "coincides with an input")
    go(I(), P(), O(live=lens.data_ptr()), "coincides with an input")
    go(I(), P(), O(mask=st2.data_ptr()), "coincides with d_state_out")
    go(I(ids=ids.data_ptr() + 4), P(ref.I64), O(), "not aligned")
    go(I(), P(), O(mask=mask.data_ptr() + 2), "not 4-byte aligned")
    go(I(index=index.data_ptr() + 2), P(), O(), "not 4-byte aligned")
    go(I(table=tab.data_ptr() + 1), P(), O(), "not 2-byte aligned")
    go(I(state=st.data_ptr() + 4), P(), O(), "not 8-byte aligned")
    for which in range(3):
        si, o, so = I(), P(), O()
        (si, o, so)[which].struct_size = 8
        go(si, o, so, "struct_size")
        (si, o, so)[which].struct_size = 4097
        go(si, o, so, "struct_size")
    huge = _ffi.SplNestIn((1 << 31), 0, None, None, st.data_ptr(), tab.data_ptr(), index.data_ptr(), S, R, n_dep, index.numel())
    go(huge, P(), O(), "n_seqs >= 2^31")

    # the index call
    n = ctypes.c_uint32(0)

    def gi(word, table=tab.data_ptr(), n_states=S, n_ret=R, n_words=nw, out=index.data_ptr(), n_dep_p=ctypes.byref(n)):
        assert L.spl_nest_index_device(tok.handle, table, n_states, n_ret, n_words, out, n_dep, n_dep_p, None) == -1, word
        assert word in _ffi.last_error(), (word, _ffi.last_error())
    gi("d_table is null", table=None)
    gi("d_index is null", out=None)
    gi("n_dep is null", n_dep_p=None)
    gi("n_states is 0", n_states=0)
    gi("n_states is 4097", n_states=4097)
    gi("n_ret is 4097", n_ret=4097)
    gi("n_words is too small", n_words=nw - 1)
    gi("n_words is above 2^26", n_words=(1 << 26) + 1)
    gi("not 2-byte aligned", table=tab.data_ptr() + 1)
    gi("not 4-byte aligned", out=index.data_ptr() + 2)
    gi("coincides with d_table", out=tab.data_ptr())
    # state out with state in is the one overlap allowed
    assert L.spl_nest_step_device(tok.handle, ctypes.byref(I()), ctypes.byref(P()), ctypes.byref(O(state=st.data_ptr())), None) == 0
    torch.cuda.synchronize()
    # the Python layer: dtypes, shapes, sizes
    s2 = st[:2].contiguous()
    kw = dict(n_states=S, n_ret=R, dep_cap=n_dep)
    with pytest.raises(ValueError, match="int32 or int64"):
        dv.nest_step_device(tok, ids.to(torch.int16), None, s2, tab, index, end_ids=[25], **kw)
    with pytest.raises(ValueError, match="END ids are needed"):
        dv.nest_step_device(tok, ids, None, s2, tab, index, end_ids=[], **kw)
    with pytest.raises(ValueError, match="at or above 32"):
        dv.nest_step_device(tok, ids, None, s2, tab, index, end_ids=[32 * nw], n_words=nw, **kw)
    with pytest.raises(ValueError, match="index must be"):
        dv.nest_step_device(tok, ids, None, s2, tab, index, end_ids=[25], n_words=nw + 4, **kw)
    with pytest.raises(ValueError, match="index must be"):
        dv.nest_step_device(tok, ids, None, s2, tab, index, end_ids=[25], n_words=nw, n_states=S, n_ret=R, dep_cap=n_dep + 1)
    with pytest.raises(ValueError, match="keep_free needs"):
        dv.nest_step_device(tok, ids, None, s2, tab, index, end_ids=[25], keep_free=True, n_words=nw, **kw)
    with pytest.raises(ValueError, match="max_depth must be"):
        dv.nest_step_device(tok, ids, None, s2, tab, index, end_ids=[25], max_depth=65, n_words=nw, **kw)
    with pytest.raises(ValueError, match=r"shape \[batch, 5\]"):
        dv.nest_step_device(tok, ids, None, st[:3].contiguous(), tab, index, end_ids=[25], n_words=nw, **kw)
    with pytest.raises(ValueError, match="table must be"):
        dv.nest_step_device(tok, ids, None, s2, tab[:100], index, end_ids=[25], n_words=nw, **kw)
    with pytest.raises(ValueError, match="n_words is too small"):
        dv.nest_index_device(tok, tab, S, R, n_words=nw - 1)
    with pytest.raises(ValueError, match="NestTable"):
        dv.nest_table((tb[0], tb[3]))
    with pytest.raises(ValueError, match="max_depth must be"):
        tok.json_guide(2, end_ids=[25], max_depth=0)
    assert dv.nest_state([0, None, 5], dev).cpu().tolist() == [[1 << 16, 0, 0, 0, 0], [0] * 5, [5 | 1 << 16, 0, 0, 0, 0]]
    out = dv.nest_step_device(tok, None, None, dv.nest_state([0, None], dev), tab, index, end_ids=[25], n_words=nw, **kw)
    assert out[0].cpu().tolist() == [[1 << 16, 0, 0, 0, 0], [0] * 5] and out[2].cpu().tolist() == [1, 0]


# ---------------------------------------------------------------------------------------------- the shipped vocabularies, end to end
_matrices = {}


def _matrix(name):
    """(tokenizer, ids [n], bytes [n, longest] zero padded, lengths [n], {id: bytes}, a special id) of a shipped vocabulary's ordinary tokens"""
    if name not in _matrices:
        from splintr_amd import Tokenizer, _ffi
        tok = Tokenizer.from_pretrained(name)
        toks, special = [], None
        for i in range(tok.vocab_size):
            p, n = ctypes.c_void_p(), ctypes.c_uint32()
            kind = _ffi.lib().spl_token_bytes(tok.handle, i, ctypes.byref(p), ctypes.byref(n))
            if kind in (1, 2) and n.value:
                toks.append((i, ctypes.string_at(p, n.value)))
            elif kind == 3 and special is None:
                special = i
        M = np.zeros((len(toks), max(len(b) for _, b in toks)), dtype=np.uint8)
        for r, (_, b) in enumerate(toks):
            M[r, :len(b)] = np.frombuffer(b, dtype=np.uint8)
        _matrices[name] = (tok, np.array([i for i, _ in toks], dtype=np.int64), M, np.array([len(b) for _, b in toks], dtype=np.int64), dict(toks), special)
    return _matrices[name]


def _np_rows(t, ids, M, lens, stride):
    """brute force over every ordinary id and every state at once: rows uint32 [S, stride] of the ids that walk stack-free and alive"""
    S = t.n_states
    # next state; S: dead (it stays dead); S + 1: touched (it stays so)
    nxt = np.where(t.op != 0, S + 1, np.where(t.trans < S, t.trans, S)).astype(np.int64)
    nxt = np.concatenate([nxt, np.full((1, 256), S, dtype=np.int64), np.full((1, 256), S + 1, dtype=np.int64)])
    rows = np.zeros((S, stride), dtype=np.uint32)
    for q in range(S):
        at = np.full(len(ids), q, dtype=np.int64)
        for j in range(M.shape[1]):
            on = np.flatnonzero((lens > j) & (at < S))
            if not len(on):
                break
            at[on] = nxt[at[on], M[on, j]]
        ok = ids[at < S]
        np.bitwise_or.at(rows[q], ok >> 5, (np.uint32(1) << (ok & 31).astype(np.uint32)))
    return rows


def _refuse(name):
    raise ValueError(name)


def _oracle(data):
    try:
        json.loads(data.decode("utf-8"), parse_constant=_refuse)
        return True
    except (ValueError, RecursionError):
        return False


def _bits_at(mask, ids):
    """bit ids[b] of row b, on the device -> a bool tensor"""
    import torch
    words = mask.gather(1, (ids >> 5).to(torch.int64).unsqueeze(1)).flatten()
    return ((words >> (ids & 31).to(torch.int32)) & 1).bool()


def _uniform(mask, gen):
    import torch
    B, nw = mask.shape
    shifts = torch.arange(32, device=mask.device, dtype=torch.int32)
    bits = ((mask.unsqueeze(-1) >> shifts) & 1).reshape(B, nw * 32).to(torch.float32)
    return torch.multinomial(bits, 1, generator=gen).flatten()


@pytest.mark.parametrize("name", ["cl100k_base", "o200k_base"])
def test_shipped_vocabulary_json_guide_end_to_end(name):
    import torch
    from splintr_amd import device as dv
    tok, ids, M, lens, by_id, special = _matrix(name)
    assert special is not None
    B, STEPS, DEPTH = 256, 24, 32
    guide = tok.json_guide(B, end_ids=[special], max_depth=DEPTH)
    t, nw, S = guide.nest, guide.n_words, guide.n_states
    assert S == 85 and guide.n_ret == 1 and guide.start == 0
    stride = ref.stride(nw)
    rows_t, dep_off_t, dep_ids_t, some_t = dv.nest_index_views(guide.index, S, nw, guide.n_dep)
    rows, some = rows_t.cpu().numpy().view(np.uint32), some_t.cpu().numpy()
    assert (rows == _np_rows(t, ids, M, lens, stride)).all()
    assert some.tolist() == (rows != 0).any(axis=1).astype(np.uint8).tolist()
    deps = cases.dep_lists(dep_off_t.cpu().numpy(), dep_ids_t.cpu().numpy())
    tab = (t.trans.tolist(), t.ret, t.op.tolist(), t.accept.tolist())             # (lists: the definition's walk, quick enough for 200 k ids)
    longest = sorted(range(S), key=lambda q: -len(deps[q]))
    for q in sorted({0, *longest[:4], *random.Random(3).sample(range(S), 4)})[:8]:
        assert deps[q] == [i for i in ids.tolist() if ref.touches(tab, q, by_id[i]) == "touch"], (name, q)
    assert guide.n_dep == sum(map(len, deps)) and 100 < len(deps[longest[0]]) < 4000
    # B sequences draw uniformly from their masks; the host walks along
    dev = guide.mask.device
    guide.begin()
    gen = torch.Generator(device=dev).manual_seed(5)
    at = [(t.start, ())] * B
    text = [b""] * B
    ended = [False] * B
    for step in range(STEPS):
        live = guide.live.cpu().numpy().astype(bool)
        assert live.tolist() == [not e for e in ended]
        pick = _uniform(guide.mask, gen)
        assert (_bits_at(guide.mask, pick) | ~guide.live.bool()).all().item()
        for b, i in enumerate(pick.cpu().tolist()):
            if ended[b]:
                continue
            if i == special:                                                   # END was in the mask: the document is whole
                assert t.ends(*at[b]) and _oracle(text[b]), (name, step, b, text[b])
                ended[b] = True
                continue
            at[b] = t.walk(at[b][0], at[b][1], by_id[i], DEPTH)
            assert at[b] is not None, (name, step, b, text[b], by_id[i])
            text[b] += by_id[i]
        guide.step(pick, guide.live.to(torch.int32))
        on = [b for b in range(B) if not ended[b]]
        q, depth, stacks = guide.q.cpu().tolist(), guide.depth.cpu().tolist(), guide.stacks()
        assert [q[b] for b in on] == [at[b][0] for b in on] and [depth[b] for b in on] == [len(at[b][1]) for b in on]
        assert [stacks[b] for b in on] == [at[b][1] for b in on]
        assert guide.done.cpu().tolist() == ended and not guide.broken.any().item()
    assert len(on) > B // 2 and max(len(at[b][1]) for b in on) >= 1 and len(set(text)) > B // 2
    # close every document now, a byte an id
    byte_id = {b[0]: i for i, b in by_id.items() if len(b) == 1}
    assert len(byte_id) == 256
    tails = [b"" if ended[b] else t.shortest_completion(*at[b], max_depth=DEPTH) for b in range(B)]
    assert all(x is not None for x in tails)
    for k in range(max(map(len, tails))):
        feed = torch.tensor([byte_id[x[k]] if k < len(x) else 0 for x in tails], dtype=torch.int64, device=dev)
        n = torch.tensor([1 if k < len(x) else 0 for x in tails], dtype=torch.int32, device=dev)
        assert (_bits_at(guide.mask, feed) | (n == 0)).all().item(), k
        guide.step(feed, n)
    assert guide.live.cpu().tolist() == [int(not e) for e in ended] and (guide.depth == 0).all().item()
    end_t = torch.full((B,), special, dtype=torch.int64, device=dev)
    assert (_bits_at(guide.mask, end_t)).all().item()                           # (a done row is ones)
    guide.step(end_t, guide.live.to(torch.int32))
    assert guide.done.all().item() and not guide.broken.any().item() and not guide.live.any().item() and (guide.mask == -1).all().item()
    for b in range(B):
        assert _oracle(text[b] + tails[b]) and (text[b] + tails[b]).lstrip()[:1] == b"{", (name, b, text[b], tails[b])


def test_nest_guide_beside_the_streaming_decode():
    import torch
    tok, ids, M, lens, by_id, special = _matrix("cl100k_base")
    B = 64
    guide = tok.json_guide(B, end_ids=[special], top="value", ws="compact", max_depth=3)
    dec = tok.device_streaming_decoder(B, skip_special_tokens=True)
    assert guide.begin() is guide.mask and guide.live.cpu().tolist() == [1] * B and guide.n_states == 119
    dev = guide.mask.device
    gen = torch.Generator(device=dev).manual_seed(11)
    texts, drawn = [""] * B, [b""] * B
    for step in range(12):
        before = guide.mask.clone()
        dec.allowed_mask(guide.mask, and_into=True)                             # the UTF-8 rows ANDed in: the table keeps strings well-formed itself
        assert ((guide.mask & ~before) == 0).all().item() and (guide.mask != 0).any(1).all().item()
        logits = torch.zeros((B, tok.vocab_size), dtype=torch.float32, device=dev)
        guide.apply(logits, live_only=True)
        pick = _uniform(guide.mask, gen)
        live = guide.live.cpu().numpy().astype(bool)
        for b, i in enumerate(pick.cpu().tolist()):
            if live[b]:
                assert logits[b, i].item() == 0.0
                drawn[b] += by_id.get(i, b"")
        lens_t = guide.live.to(torch.int32)
        out = dec.add_tokens(pick.to(torch.int32), lens_t)
        texts = [a + (o or "") for a, o in zip(texts, out)]
        guide.step(pick, lens_t)
        assert not dec.stalled.any().item(), "a sequence stalled"
    assert not guide.broken.any().item() and (guide.depth <= 3).all().item()
    t = guide.nest
    for b in range(B):
        got = texts[b].encode("utf-8")
        assert drawn[b].startswith(got) and len(drawn[b]) - len(got) < 4, (b, drawn[b], got)
        at = t.walk(t.start, (), drawn[b], 3)
        assert at is not None
        if guide.done.cpu().tolist()[b]:
            assert _oracle(drawn[b])
        else:
            assert _oracle(drawn[b] + t.shortest_completion(*at, max_depth=3)), (b, drawn[b])
    guide.begin(rows=[7])
    assert guide.live.cpu().tolist()[7] == 1 and guide.state.cpu().tolist()[7] == [1 << 16, 0, 0, 0, 0]
    guide.reset([7])
    assert guide.state.cpu().tolist()[7] == [0] * 5 and (guide.mask[7] == -1).all().item()


def test_ops_zero_table_beside_the_regex_guide():
    import torch
    from splintr_amd import dfa, nest
    tok, ids, M, lens, by_id, special = _matrix("cl100k_base")
    d = dfa.compile_regex(r"\d{4}-\d{2}-\d{2}")
    B = 64
    rx = tok.regex_guide(B, d, end_ids=[special])
    ng = tok.nest_guide(B, nest.from_dfa(d), end_ids=[special])
    assert ng.n_dep == 0 and ng.n_ret == 0
    rx.begin()
    ng.begin()
    gen = torch.Generator(device=rx.mask.device).manual_seed(2)
    for step in range(12):
        assert torch.equal(rx.mask, ng.mask) and torch.equal(rx.state, ng.state[:, 0]) and torch.equal(rx.live, ng.live)
        assert (ng.state[:, 1:] == 0).all().item()
        if not rx.live.any().item():
            break
        pick = _uniform(rx.mask, gen)
        n = rx.live.to(torch.int32)
        rx.step(pick, n)
        ng.step(pick, n)
    assert rx.done.all().item() and ng.done.all().item()
