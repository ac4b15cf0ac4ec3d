"""GPU tests (-m gpu): spl_dfa_draft_device and spl_nest_draft_device -- draft verification for the regex and nest guides -- through the C
ABI into guarded buffers against the definition of tests/draft_ref.py: the checks of tests/draft_cases.py, batch sizes around the grid's
edges, a mask base off its 16-byte alignment, every refusal by its message, the shipped vocabularies with json_guide and a regex_guide
pattern against K + 1 (or per-path) calls of the existing step, and a speculative loop end to end beside a plain guide."""
import ctypes
import json
import random

import numpy as np
import pytest

import dfa_cases
import dfa_ref
import draft_cases as cases
import draft_ref as ref
import nest_cases
import nest_ref
import vocabgen

pytestmark = pytest.mark.gpu

WORD_POISON = 0x5A5A5A5A5A5A5A5A
MASK_POISON = 0x5A5A5A5A
PATTERN = r"[a-z]+|\s+|[^a-z\s]+"

_toks, _shipped, _indexes = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release_the_tokenizers():
    """The tokenizers this module keeps (and the streams their pipelines picked: hardware queues are few) go with the module, not with the
    process: what runs behind it finds the GPU's queues as this module found them."""
    yield
    import gc
    import torch
    _indexes.clear()
    _toks.clear()
    _shipped.clear()
    gc.collect()
    torch.cuda.synchronize()


def _toy(name, tmp_path_factory):
    if name not in _toks:
        from splintr_amd import Tokenizer
        vocab, specials, _ = cases.vocab(name)
        path = tmp_path_factory.mktemp("draft") / (name + ".tiktoken")
        path.write_bytes(vocabgen.tiktoken({b: i for i, b in vocab.items()}))
        _toks[name] = Tokenizer(str(path), PATTERN, {v.decode(): k for k, v in specials.items()})
    return _toks[name]


def _index(tok, kind, table, n_states, n_ret, n_words):
    """(table on the device, index, dep_cap) by the library's own index build, kept per table"""
    import torch
    from splintr_amd import device as dv
    key = (id(tok), kind, np.asarray(table).tobytes(), n_words)
    if key not in _indexes:
        t_tab = torch.from_numpy(np.ascontiguousarray(table, dtype=np.uint8)).to(torch.device("cuda", 0))
        if kind == "dfa":
            _indexes[key] = (t_tab, dv.dfa_index_device(tok, t_tab, n_states, n_words=n_words), 0)
        else:
            index, n_dep = dv.nest_index_device(tok, t_tab, n_states, n_ret, n_words=n_words)
            _indexes[key] = (t_tab, index, n_dep)
    return _indexes[key]


def _structs(tok, kind, table, n_states, n_ret, t_ids, t_len, t_sin, flags, end_ids, n_words, max_depth):
    from splintr_amd import _ffi
    t_tab, t_index, dep_cap = _index(tok, kind, table, n_states, n_ret, n_words)
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    B, K = t_ids.shape
    if kind == "dfa":
        return _ffi.SplDfaIn(B, K, ptr(t_ids), ptr(t_len), t_sin.data_ptr(), t_tab.data_ptr(), t_index.data_ptr(), n_states), _ffi.SplDfaOpts(flags, n_words, end_ids)
    return (_ffi.SplNestIn(B, K, ptr(t_ids), ptr(t_len), t_sin.data_ptr(), t_tab.data_ptr(), t_index.data_ptr(), n_states, n_ret, dep_cap, t_index.numel()),
            _ffi.SplNestOpts(flags, n_words, end_ids, max_depth))


def _draft(tok, kind, table, n_states, n_ret, *, ids, state, parent=None, lengths=None, flags=0, end_ids=(), n_words, max_depth=64, mask_init=None,
           want_live=True, want_state=True, off16=0):
    """One draft call through the C ABI with poisoned outputs and a spare row behind each -> dict of numpy arrays; asserts that nothing
    behind or around the rows was written, that state_in is byte-equal before and after, that outputs that are not wanted stay untouched
    and that KEEP_FREE left the rows of nodes that are not constrained alone.  off16: words the mask base lies behind a 16-byte boundary."""
    import torch
    from splintr_amd import _ffi
    dev = torch.device("cuda", 0)
    ids = np.ascontiguousarray(ids)
    B, K = ids.shape
    R, W = 1 + K, (1 if kind == "dfa" else nest_ref.STATE_WORDS)
    if ids.dtype == np.int64:
        flags |= dfa_ref.I64
    t_ids = torch.from_numpy(ids.view(np.int32) if ids.dtype == np.uint32 else ids).to(dev)
    t_len = None if lengths is None else torch.from_numpy(np.ascontiguousarray(lengths, dtype=np.int32)).to(dev)
    rows_in = np.concatenate([np.asarray(state, dtype=np.uint64).reshape(B, W), np.full((1, W), WORD_POISON, dtype=np.uint64)])
    t_sin = torch.from_numpy(rows_in.view(np.int64)).to(dev)
    t_par, dflags = None, 0
    if parent is not None:
        parent = np.ascontiguousarray(parent, dtype=np.int32)
        t_par = torch.from_numpy(parent).to(dev)
        dflags = _ffi.SPL_DRAFT_PARENT_PER_SEQ if parent.ndim == 2 and parent.size else 0       # (no node: no row of parents to point at)
    n = B * R
    t_sout = torch.full((n + 1, W), WORD_POISON, dtype=torch.int64, device=dev)
    flat = torch.full(((n + 1) * n_words + 4,), MASK_POISON, dtype=torch.int32, device=dev)
    t_mask = flat[off16:off16 + (n + 1) * n_words].view(n + 1, n_words)
    assert t_mask.data_ptr() % 16 == 4 * off16
    init = None
    if mask_init is not None:
        init = np.asarray(mask_init, dtype=np.uint32).reshape(n, n_words)
        t_mask[:n] = torch.from_numpy(init.view(np.int32)).to(dev)
    t_live = torch.full((n + 1,), 0x5A, dtype=torch.uint8, device=dev)
    t_ok = torch.full((B * K + 1,), 0x5A, dtype=torch.uint8, device=dev)
    si, o = _structs(tok, kind, table, n_states, n_ret, t_ids, t_len, t_sin, flags, end_ids, n_words, max_depth)
    d = _ffi.SplDraftOut(dflags, t_par.data_ptr() if t_par is not None and t_par.numel() else None, t_mask.data_ptr(), t_ok.data_ptr(),
                         t_live.data_ptr() if want_live else None, t_sout.data_ptr() if want_state else None)
    fn = _ffi.lib().spl_dfa_draft_device if kind == "dfa" else _ffi.lib().spl_nest_draft_device
    rc = fn(tok.handle, ctypes.byref(si), ctypes.byref(o), ctypes.byref(d), torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, _ffi.last_error()
    st = t_sout.cpu().numpy().view(np.uint64)
    whole = flat.cpu().numpy().view(np.uint32)
    mask = whole[off16:off16 + (n + 1) * n_words].reshape(n + 1, n_words)
    live, ok = t_live.cpu().numpy(), t_ok.cpu().numpy()
    assert (t_sin.cpu().numpy().view(np.uint64) == rows_in).all(), "state_in was written"
    assert (st[n] == WORD_POISON).all() and (mask[n] == MASK_POISON).all() and live[n] == 0x5A and ok[B * K] == 0x5A, "written behind the rows"
    assert (whole[:off16] == MASK_POISON).all() and (whole[off16 + (n + 1) * n_words:] == MASK_POISON).all(), "written around the mask"
    assert (ok[:B * K] <= 1).all()
    if not want_live:
        assert (live == 0x5A).all()
    elif flags & dfa_ref.KEEP_FREE:
        keep = live[:n] == 0
        assert (mask[:n][keep] == (init[keep] if init is not None else MASK_POISON)).all(), "KEEP_FREE: a row that is not constrained was written"
    if not want_state:
        assert (st == WORD_POISON).all()
    shape = (B, R) if kind == "dfa" else (B, R, W)
    return dict(mask=mask[:n].reshape(B, R, n_words).copy(), ok=ok[:B * K].reshape(B, K).copy(), live=live[:n].reshape(B, R).copy() if want_live else None,
                state=st[:n].reshape(shape).copy() if want_state else None)


def _drafter(tok, **fixed):
    return lambda kind, table, n_states, n_ret, **kw: _draft(tok, kind, table, n_states, n_ret, **dict(fixed, **kw))


def _stepper(tok):
    """one call of the existing step through the Python layer -> dict of numpy arrays"""
    import torch
    from splintr_amd import device as dv

    def step(kind, table, n_states, n_ret, *, ids, state, lengths=None, end_ids, n_words, max_depth=64):
        dev = torch.device("cuda", 0)
        t_tab, t_index, dep_cap = _index(tok, kind, table, n_states, n_ret, n_words)
        ids = np.ascontiguousarray(ids)
        t_ids = torch.from_numpy(ids.view(np.int32) if ids.dtype == np.uint32 else ids).to(dev)
        t_len = None if lengths is None else torch.from_numpy(np.ascontiguousarray(lengths, dtype=np.int32)).to(dev)
        t_st = torch.from_numpy(np.ascontiguousarray(state, dtype=np.uint64).view(np.int64)).to(dev)
        if kind == "dfa":
            s, m, l = dv.dfa_step_device(tok, t_ids, t_len, t_st, t_tab, t_index, end_ids=list(end_ids), n_states=n_states, n_words=n_words)
        else:
            s, m, l = dv.nest_step_device(tok, t_ids, t_len, t_st, t_tab, t_index, n_states=n_states, n_ret=n_ret, dep_cap=dep_cap, end_ids=list(end_ids),
                                          max_depth=max_depth, n_words=n_words)
        return dict(state=s.cpu().numpy().view(np.uint64), mask=m.cpu().numpy().view(np.uint32), live=l.cpu().numpy())
    return step


# ---------------------------------------------------------------------------------------------- the shared checks
@pytest.mark.parametrize("name", sorted(dfa_cases.TOYS))
def test_anchor_against_the_step(name, tmp_path_factory):
    tok = _toy(name, tmp_path_factory)
    cases.check_anchor(_drafter(tok), _stepper(tok), name)


def test_anchor_with_a_stack(tmp_path_factory):
    tok = _toy("brackets", tmp_path_factory)
    cases.check_anchor(_drafter(tok), _stepper(tok), "brackets", kinds=("nest",))


def test_topologies(tmp_path_factory):
    cases.check_topologies(_drafter(_toy("gaps", tmp_path_factory)), "gaps", kinds=("dfa",))
    cases.check_topologies(_drafter(_toy("brackets", tmp_path_factory)), "brackets", kinds=("nest",))


def test_orphans_lengths_ids_and_input_states(tmp_path_factory):
    d, b = _drafter(_toy("gaps", tmp_path_factory)), _drafter(_toy("brackets", tmp_path_factory))
    for check in (cases.check_orphans, cases.check_lengths, cases.check_order, cases.check_rejected, cases.check_done_child):
        check(d)
        check(b, "brackets", "nest")
    cases.check_input_states(lambda kind, *a, **kw: (d if kind == "dfa" else b)(kind, *a, **kw))


def test_stack_and_dependent_ids(tmp_path_factory):
    cases.check_stack(_drafter(_toy("brackets", tmp_path_factory)))
    cases.check_deps(_drafter(_toy("deps", tmp_path_factory)))
    cases.check_deps(_drafter(_toy("deps", tmp_path_factory), off16=1))


def test_layouts_and_flags(tmp_path_factory):
    for off16 in (0, 1, 3):                                            # a mask base 0, 4 and 12 bytes behind a 16-byte boundary
        d, b = _drafter(_toy("gaps", tmp_path_factory), off16=off16), _drafter(_toy("brackets", tmp_path_factory), off16=off16)
        cases.check_layout_and_flags(lambda kind, *a, **kw: (d if kind == "dfa" else b)(kind, *a, **kw))


@pytest.mark.parametrize("B", [0, 1, 63, 64, 65, 1025])
def test_batch_sizes(B, tmp_path_factory):
    rng = random.Random(B)
    tree = [-1, 0, 0]
    for name, kind in (("gaps", "dfa"), ("brackets", "nest")):
        c = cases.Case(name)
        tab = c.tab(kind)
        states = [s if b % 7 else cases._r(kind).FREE for b, s in enumerate(c.starts(kind, B))]
        ids = [[rng.choice(c.pool[:12]) for _ in range(3)] for _ in range(B)]
        r, _ = cases.expect(_drafter(_toy(name, tmp_path_factory)), kind, c.toks, tab, cases.raw_of(kind, states), states,
                            np.array(ids, dtype=np.int64).reshape(B, 3), tree, c.nw, c.end)
        assert r["ok"].shape == (B, 3)


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals(tmp_path_factory):
    import torch
    from splintr_amd import _ffi, device as dv, nest
    tok = _toy("brackets", tmp_path_factory)
    c = cases.Case("brackets")
    L = _ffi.lib()
    dev = torch.device("cuda", 0)
    nw = c.nw
    tb = c.nest
    t = nest.NestTable(tb[0], tb[2], tb[1], tb[3])
    S, R = t.n_states, t.n_ret
    ids = torch.zeros((2, 3), dtype=torch.int32, device=dev)
    lens = torch.ones(2, dtype=torch.int32, device=dev)
    par = torch.tensor([-1, 0, 1], dtype=torch.int32, device=dev)
    st = torch.zeros((2, 5), dtype=torch.int64, device=dev)
    so = torch.zeros((8, 5), dtype=torch.int64, device=dev)
    mask = torch.zeros((8, nw), dtype=torch.int32, device=dev)
    live = torch.zeros(16, dtype=torch.uint8, device=dev)
    ok = torch.zeros(16, dtype=torch.uint8, device=dev)
    tab = dv.nest_table(t, dev)
    index, n_dep = dv.nest_index_device(tok, tab, S, R, n_words=nw)
    d_tab = dv.dfa_table((tb[0], tb[3]), dev)
    d_index = dv.dfa_index_device(tok, d_tab, S, n_words=nw)
    s1 = torch.zeros(2, dtype=torch.int64, device=dev)

    def I(kind, **kw):
        if kind == "dfa":
            return _ffi.SplDfaIn(kw.get("n_seqs", 2), kw.get("row_len", 3), kw.get("ids", ids.data_ptr()), kw.get("lens", lens.data_ptr()),
                                 kw.get("state", s1.data_ptr()), kw.get("table", d_tab.data_ptr()), kw.get("index", d_index.data_ptr()), kw.get("n_states", S))
        return _ffi.SplNestIn(kw.get("n_seqs", 2), kw.get("row_len", 3), kw.get("ids", ids.data_ptr()), kw.get("lens", lens.data_ptr()),
                              kw.get("state", st.data_ptr()), kw.get("table", tab.data_ptr()), kw.get("index", index.data_ptr()), kw.get("n_states", S),
                              kw.get("n_ret", R), kw.get("dep_cap", n_dep), kw.get("index_bytes", index.numel()))

    def P(kind, flags=0, n_words=nw, end=(25,), max_depth=8):
        return _ffi.SplDfaOpts(flags, n_words, end) if kind == "dfa" else _ffi.SplNestOpts(flags, n_words, end, max_depth)

    D = lambda **kw: _ffi.SplDraftOut(kw.get("flags", 0), kw.get("parent", par.data_ptr()), kw.get("mask", mask.data_ptr()), kw.get("ok", ok.data_ptr()),
                                      kw.get("live", live.data_ptr()), kw.get("state", so.data_ptr()))

    for kind, fn, who in (("dfa", L.spl_dfa_draft_device, "spl_dfa_draft_device"), ("nest", L.spl_nest_draft_device, "spl_nest_draft_device")):
        def go(si, o, d, word):
            assert fn(tok.handle, ctypes.byref(si) if si else None, ctypes.byref(o) if o else None, ctypes.byref(d) if d else None, None) == -1, word
            assert who in _ffi.last_error() and word in _ffi.last_error(), (word, _ffi.last_error())
        i, p = (lambda **kw: I(kind, **kw)), (lambda *a, **kw: P(kind, *a, **kw))
        # everything the step refuses
        go(None, p(), D(), "the input struct is null")
        go(i(), None, D(), "the options are null")
        go(i(), p(), None, "the draft struct is null")
        go(i(table=None), p(), D(), "d_table is null")
        go(i(index=None), p(), D(), "d_index is null")
        go(i(state=None), p(), D(), "d_state_in is null")
        go(i(ids=None), p(), D(), "d_ids is null")
        go(i(n_states=0), p(), D(), "n_states is 0")
        go(i(n_states=4097), p(), D(), "n_states is 4097")
        go(i(), p(n_words=nw - 1), D(), "n_words is too small")
        go(i(), p(n_words=(1 << 26) + 1), D(), "n_words is above 2^26")
        go(i(), p(1), D(), "unknown flag bit")
        go(i(), p(end=()), D(), "n_end is 0")
        go(i(), p(end=(3, 32 * nw)), D(), "at or above 32 * n_words")
        go(i(ids=ids.data_ptr() + 4), p(dfa_ref.I64), D(), "not aligned")
        go(i(), p(), D(mask=mask.data_ptr() + 2), "not 4-byte aligned")
        go(i(), p(), D(state=so.data_ptr() + 4), "not 8-byte aligned")
        go(i(n_seqs=1 << 31, row_len=0, ids=None, lens=None), p(), D(), "n_seqs >= 2^31")
        if kind == "nest":
            go(i(n_ret=4097), p(), D(), "n_ret is 4097")
            go(i(), p(max_depth=0), D(), "max_depth is 0")
            go(i(), p(max_depth=65), D(), "max_depth is 65")
            go(i(dep_cap=n_dep + 1), p(), D(), "the index is too small for dep_cap")
        for which in range(3):
            si, o, d = i(), p(), D()
            (si, o, d)[which].struct_size = 8
            go(si, o, d, "struct_size")
        # the draft's own
        go(i(row_len=65), p(), D(), "row_len is 65, above SPL_DRAFT_MAX_NODES (64)")
        go(i(), p(), D(ok=None), "d_ok is null")
        go(i(), p(), D(mask=None), "d_mask is null")
        go(i(), p(), D(parent=par.data_ptr() + 2), "d_parent is not 4-byte aligned")
        go(i(), p(), D(flags=1, parent=None), "SPL_DRAFT_PARENT_PER_SEQ without d_parent")
        go(i(), p(), D(flags=2), "unknown draft flag bit")
        go(i(n_seqs=(1 << 31) // 4, row_len=3), p(), D(), "(1 + row_len) * n_seqs >= 2^31")
        go(i(n_seqs=((1 << 31) + 64) // 65, row_len=64), p(), D(), "(1 + row_len) * n_seqs >= 2^31")
        state_in = s1 if kind == "dfa" else st
        for name, other in (("d_mask", ids), ("d_ok", lens), ("d_live", d_tab if kind == "dfa" else tab), ("d_state_out", state_in), ("d_mask", state_in),
                            ("d_ok", d_index if kind == "dfa" else index), ("d_live", par)):
            go(i(), p(), D(**{name[2:].replace("state_out", "state"): other.data_ptr()}), name + " coincides with an input array")
        go(i(), p(), D(ok=mask.data_ptr()), "d_ok coincides with d_mask")
        go(i(), p(), D(live=ok.data_ptr()), "d_live coincides with d_ok")
        go(i(), p(), D(state=mask.data_ptr()), "d_mask coincides with d_state_out")
        # live and the state rows may be absent, the parents too; an empty batch and an empty draft pass
        assert fn(tok.handle, ctypes.byref(i()), ctypes.byref(p()), ctypes.byref(D(live=None, state=None, parent=None)), None) == 0, _ffi.last_error()
        assert fn(tok.handle, ctypes.byref(i(n_seqs=0)), ctypes.byref(p()), ctypes.byref(D()), None) == 0, _ffi.last_error()
        assert fn(tok.handle, ctypes.byref(i(row_len=0, ids=None)), ctypes.byref(p()), ctypes.byref(D(parent=None)), None) == 0, _ffi.last_error()
    torch.cuda.synchronize()
    # the Python layer
    kw = dict(n_states=S, n_ret=R, dep_cap=n_dep, end_ids=[25], n_words=nw)
    with pytest.raises(ValueError, match="at most 64 nodes"):
        dv.nest_draft_device(tok, torch.zeros((2, 65), dtype=torch.int32, device=dev), None, st, tab, index, **kw)
    with pytest.raises(ValueError, match="parent must be"):
        dv.nest_draft_device(tok, ids, None, st, tab, index, parent=par.to(torch.int64), **kw)
    with pytest.raises(ValueError, match="device of the ids"):
        dv.nest_draft_device(tok, ids, None, st, tab, index, parent=par.cpu(), **kw)
    with pytest.raises(ValueError, match="keep_free needs"):
        dv.dfa_draft_device(tok, ids, None, s1, d_tab, d_index, end_ids=[25], n_words=nw, keep_free=True)
    with pytest.raises(ValueError, match=r"shape \[batch, 5\]"):
        dv.nest_draft_device(tok, ids, None, s1, tab, index, **kw)
    r = dv.nest_draft_device(tok, ids, None, dv.nest_state([0, None], dev), tab, index, parent=par, states=True, **kw)
    assert r.mask.shape == (2, 4, nw) and r.ok.shape == (2, 3) and r.live.shape == (2, 4) and r.state.shape == (2, 4, 5) and r.tree
    assert r.ok.cpu().tolist()[1] == [1, 1, 1] and r.live.cpu().tolist()[1] == [0] * 4
    with pytest.raises(ValueError, match="a chain's"):
        r.accepted_len()
    r = dv.dfa_draft_device(tok, ids[:, :0].contiguous(), None, s1, d_tab, d_index, end_ids=[25], n_words=nw)
    assert r.mask.shape == (2, 1, nw) and r.ok.shape == (2, 0) and r.state is None and r.accepted_len().tolist() == [0, 0]


# ---------------------------------------------------------------------------------------------- the shipped vocabularies
def _ship(name):
    if name not in _shipped:
        from splintr_amd import Tokenizer, _ffi
        tok = Tokenizer.from_pretrained(name)
        by_id, special = {}, None
        for i in range(tok.vocab_size):
            p, n = ctypes.c_void_p(), ctypes.c_uint32()
            kind = _ffi.lib().spl_token_bytes(tok.handle, i, ctypes.byref(p), ctypes.byref(n))
            if kind in (1, 2) and n.value:
                by_id[i] = ctypes.string_at(p, n.value)
            elif kind == 3 and special is None:
                special = i
        _shipped[name] = (tok, by_id, special)
    return _shipped[name]


def _uniform(mask, gen):
    import torch
    B, nw = mask.shape
    shifts = torch.arange(32, device=mask.device, dtype=torch.int32)
    bits = ((mask.unsqueeze(-1) >> shifts) & 1).reshape(B, nw * 32).to(torch.float32)
    return torch.multinomial(bits, 1, generator=gen).flatten()


def _bits_at(mask, ids):
    import torch
    words = mask.gather(1, (ids >> 5).to(torch.int64).unsqueeze(1)).flatten()
    return ((words >> (ids & 31).to(torch.int32)) & 1).bool()


def _step_copy(guide, ids, lengths):
    """the existing step over a COPY of the guide's state -> (state, mask, live); the guide does not move"""
    from splintr_amd import device as dv
    if guide.state.dim() == 1:
        return dv.dfa_step_device(guide._tok, ids, lengths, guide.state.clone(), guide.table, guide.index, end_ids=guide.end_ids, n_states=guide.n_states,
                                  n_words=guide.n_words)
    return dv.nest_step_device(guide._tok, ids, lengths, guide.state.clone(), guide.table, guide.index, n_states=guide.n_states, n_ret=guide.n_ret,
                               dep_cap=guide.n_dep, end_ids=guide.end_ids, max_depth=guide.max_depth, n_words=guide.n_words)


def _paths(parent, K):
    return [ref.path(parent, i) for i in range(K)]


def _check_against_steps(guide, ids, parent, gen_free):
    """every mask row, ok, live and state of guide.draft(ids, parent=...) against one call of the existing step per row over a copy of the
    state, fed the node's path"""
    import torch
    B, K = ids.shape
    dev = ids.device
    before = guide.state.clone()
    t_par = None if parent is None else torch.tensor(parent, dtype=torch.int32, device=dev)
    d = guide.draft(ids, parent=t_par, states=True)
    assert torch.equal(guide.state, before), "draft moved the guide"
    word0 = (lambda s: s if s.dim() == 1 else s[:, 0])
    free = (word0(before) >> 16) & 7 == 0
    s0, m0, l0 = _step_copy(guide, None, None)
    assert torch.equal(d.mask[:, 0], m0) and torch.equal(d.live[:, 0], l0) and torch.equal(d.state[:, 0], s0)
    lives = {-1: l0}
    for i, path in enumerate(_paths(parent, K)):
        fed = ids[:, path].contiguous()
        s, m, l = _step_copy(guide, fed, torch.full((B,), len(path), dtype=torch.int32, device=dev))
        assert torch.equal(d.mask[:, 1 + i], m), i
        assert torch.equal(d.live[:, 1 + i], l) and torch.equal(d.state[:, 1 + i], s), i
        lives[i] = l
        up = lives[path[-2] if len(path) > 1 else -1]
        done = ((word0(s) >> 18) & 1).bool()
        want = l.bool() | (done & up.bool()) | free                    # (trimmed tables: a constrained state always has something to draw)
        assert torch.equal(d.ok[:, i].bool(), want), (i, d.ok[:, i].tolist(), want.tolist())
    return d


def _draw_draft(guide, parent, K, gen, rng, p_bad, vocab_size):
    """ids [B, K]: a node's id is drawn uniformly from the mask the existing step gives behind its parent's path, then overwritten with a
    uniformly random vocabulary id with probability p_bad"""
    import torch
    B, dev = guide.batch_size, guide.mask.device
    ids = torch.zeros((B, K), dtype=torch.int64, device=dev)
    for i, path in enumerate(_paths(parent, K)):
        up = path[:-1]
        _, m, _ = _step_copy(guide, ids[:, up].contiguous() if up else None, torch.full((B,), len(up), dtype=torch.int32, device=dev) if up else None)
        pick = _uniform(m, gen)
        bad = torch.tensor([rng.random() < p_bad for _ in range(B)], device=dev)
        junk = torch.tensor([rng.randrange(vocab_size) for _ in range(B)], dtype=torch.int64, device=dev)
        ids[:, i] = torch.where(bad, junk, pick)
    return ids


REGEX = r'\{"name": "[a-z ]{1,40}", "tags": \["[a-z]{1,12}"(, "[a-z]{1,12}"){0,5}\]\}'


@pytest.mark.parametrize("name", ["cl100k_base", "o200k_base"])
@pytest.mark.parametrize("which", ["json", "regex"])
def test_shipped_vocabulary_drafts_against_the_step(name, which):
    import torch
    tok, by_id, special = _ship(name)
    B = 64
    guide = tok.json_guide(B, end_ids=[special], max_depth=32) if which == "json" else tok.regex_guide(B, REGEX, end_ids=[special])
    dev = guide.mask.device
    gen = torch.Generator(device=dev).manual_seed(7)
    rng = random.Random(7)
    guide.begin()
    for _ in range(8):                                                 # eight uniformly drawn steps: stacks are no longer trivial
        guide.step(_uniform(guide.mask, gen), guide.live.to(torch.int32))
    if which == "json":
        assert int(guide.depth.max()) >= 1
    assert guide.live.any().item()
    for parent, K in ((None, 4), (cases.binary(7), 7)):
        ids = _draw_draft(guide, parent if parent is not None else cases.chain(K), K, gen, rng, 0.2, tok.vocab_size)
        d = _check_against_steps(guide, ids, parent, gen)
        assert 0 < int(d.ok.sum()) < B * K
        if parent is None:
            assert (d.ok[:, 1:] <= d.ok[:, :-1]).all().item() and torch.equal(d.accepted_len(), d.ok.sum(1))
        d32 = guide.draft(ids.to(torch.int32), parent=None if parent is None else torch.tensor([parent] * B, dtype=torch.int32, device=dev))
        assert torch.equal(d32.mask, d.mask) and torch.equal(d32.ok, d.ok) and d32.state is None
        kf = guide.draft(ids, parent=None if parent is None else torch.tensor(parent, dtype=torch.int32, device=dev), keep_free=True)
        assert torch.equal(kf.mask, d.mask) and torch.equal(kf.live, d.live)      # (rows that are not written hold ones, as the rows that are)


def test_speculative_loop_end_to_end():
    import torch
    tok, by_id, special = _ship("cl100k_base")
    B, K, ROUNDS, DEPTH = 64, 4, 8, 32
    guide = tok.json_guide(B, end_ids=[special], max_depth=DEPTH)
    plain = tok.json_guide(B, end_ids=[special], max_depth=DEPTH)      # fed exactly the accepted ids, one step at a time
    shadow = tok.json_guide(B, end_ids=[special], max_depth=DEPTH)     # the proposer's
    t = guide.nest
    dev = guide.mask.device
    gen = torch.Generator(device=dev).manual_seed(3)
    rng = random.Random(3)
    V = tok.vocab_size
    guide.begin()
    plain.begin()
    text = [b""] * B
    per_round = []
    rows = torch.arange(B, device=dev)
    for rnd in range(ROUNDS):
        shadow.state.copy_(guide.state)
        shadow.step(None)
        drafted = torch.zeros((B, K), dtype=torch.int64, device=dev)
        forbidden = torch.zeros((B, K), dtype=torch.bool, device=dev)  # a corrupted id that the shadow's mask forbids
        for k in range(K):
            pick = _uniform(shadow.mask, gen)
            bad = torch.tensor([rng.random() < 0.3 for _ in range(B)], device=dev)
            junk = torch.tensor([rng.randrange(V) for _ in range(B)], dtype=torch.int64, device=dev)
            drafted[:, k] = torch.where(bad, junk, pick)
            forbidden[:, k] = bad & ~_bits_at(shadow.mask, drafted[:, k]) & shadow.live.bool()
            shadow.step(drafted[:, k].contiguous(), shadow.live.to(torch.int32))
        d = guide.draft(drafted)
        n = d.accepted_len()
        first_bad = torch.where(forbidden.any(1), forbidden.to(torch.int64).argmax(1), torch.full((B,), K, device=dev))
        assert (n <= first_bad).all().item(), "a corrupted id the shadow's mask forbids was counted as accepted"
        logits = torch.zeros((B * (1 + K), V), dtype=torch.bfloat16, device=dev)
        assert guide.apply(logits, mask=d.mask) is logits
        shifts = torch.arange(32, device=dev, dtype=torch.int32)
        allowed = ((d.mask.view(B * (1 + K), -1).unsqueeze(-1) >> shifts) & 1).reshape(B * (1 + K), -1)[:, :V].bool()
        assert (logits[allowed] == 0).all().item() and torch.isneginf(logits[~allowed]).all().item() and (~allowed).any().item()
        bonus = _uniform(d.mask[rows, n], gen)                         # drawn under the mask behind the accepted prefix
        fed = torch.cat([drafted, torch.zeros((B, 1), dtype=torch.int64, device=dev)], 1)
        fed[rows, n] = bonus
        live = guide.live.bool()
        count = torch.where(live, n + 1, torch.zeros_like(n)).to(torch.int32)
        guide.accept(fed, count)
        read = []
        for k in range(K + 1):                                         # the plain guide: the same ids one step at a time
            read.append(((count > k) & plain.live.bool()).cpu().tolist())       # (an id behind END is not read)
            plain.step(fed[:, k].contiguous(), (count > k).to(torch.int32))
        assert torch.equal(guide.state, plain.state) and torch.equal(guide.mask, plain.mask) and torch.equal(guide.live, plain.live), rnd
        assert not guide.broken.any().item()
        fed_h = fed.cpu().tolist()
        for b in range(B):
            text[b] += b"".join(by_id.get(fed_h[b][k], b"") for k in range(K + 1) if read[k][b])
        per_round.append(float(n[live].float().mean()) if live.any().item() else 0.0)
    assert 0.5 < sum(per_round) / len(per_round) <= K, per_round
    # close every document now, a byte an id, then END
    byte_id = {b[0]: i for i, b in by_id.items() if len(b) == 1}
    stacks, q, done = guide.stacks(), guide.q.cpu().tolist(), guide.done.cpu().tolist()
    tails = [b"" if done[b] else t.shortest_completion(q[b], stacks[b], max_depth=DEPTH) for b in range(B)]
    assert all(x is not None for x in tails)
    for k in range(max(map(len, tails))):
        feed = torch.tensor([byte_id[x[k]] if k < len(x) else 0 for x in tails], dtype=torch.int64, device=dev)
        cnt = torch.tensor([1 if k < len(x) else 0 for x in tails], dtype=torch.int32, device=dev)
        assert (_bits_at(guide.mask, feed) | (cnt == 0)).all().item(), k
        guide.accept(feed, cnt)
    guide.accept(torch.full((B,), special, dtype=torch.int64, device=dev), guide.live.to(torch.int32))
    assert guide.done.all().item() and not guide.broken.any().item()
    for b in range(B):
        doc = text[b] + tails[b]
        json.loads(doc.decode("utf-8"))
        assert doc.lstrip()[:1] == b"{", (b, doc)


def test_accept_node_adopts_a_tree_node():
    import torch
    tok, by_id, special = _ship("cl100k_base")
    B = 16
    guide = tok.json_guide(B, end_ids=[special], max_depth=32)
    other = tok.json_guide(B, end_ids=[special], max_depth=32)
    dev = guide.mask.device
    gen = torch.Generator(device=dev).manual_seed(9)
    guide.begin()
    for _ in range(4):
        guide.step(_uniform(guide.mask, gen), guide.live.to(torch.int32))
    parent = cases.binary(7)
    ids = _draw_draft(guide, parent, 7, gen, random.Random(9), 0.0, tok.vocab_size)
    with pytest.raises(ValueError, match="states=True"):
        guide.accept_node(guide.draft(ids, parent=torch.tensor(parent, dtype=torch.int32, device=dev)), [0] * B)
    d = guide.draft(ids, parent=torch.tensor(parent, dtype=torch.int32, device=dev), states=True)
    node = [(-1, 0, 4, 6)[b % 4] for b in range(B)]
    with pytest.raises(ValueError, match="node must be in"):
        guide.accept_node(d, [7] * B)
    other.state.copy_(guide.state)
    ids_h = ids.cpu().tolist()
    paths = [[ids_h[b][j] for j in ref.path(parent, n)] if n >= 0 else [] for b, n in enumerate(node)]
    feed = torch.tensor([x + [0] * (3 - len(x)) for x in paths], dtype=torch.int64, device=dev)
    other.step(feed, torch.tensor([len(x) for x in paths], dtype=torch.int32, device=dev))          # the ordinary step, fed each sequence's path
    assert guide.accept_node(d, torch.tensor(node, device=dev)) is guide.mask
    assert torch.equal(guide.state, other.state) and torch.equal(guide.mask, other.mask) and torch.equal(guide.live, other.live)
