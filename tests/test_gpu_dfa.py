"""GPU tests (-m gpu): spl_dfa_index_device and spl_dfa_step_device -- the regex guide, allowed-token bitmasks from a byte DFA -- through the
C ABI into guarded buffers against the definition of tests/dfa_ref.py: the checks of tests/dfa_cases.py over the toy vocabularies, batch
sizes and vocabulary sizes around the kernels' edges, a mask base and an index base off their 16-byte alignment, the refusals, the shipped
vocabularies end to end against a numpy brute force with a uniform sampler, RegexGuide beside the streaming decode and its UTF-8 mask, and
a stacked two-pattern batch."""
import ctypes
import random
import re

import numpy as np
import pytest

import dfa_cases as cases
import dfa_ref as ref
import vocabgen

pytestmark = pytest.mark.gpu

WORD_POISON = 0x5A5A5A5A5A5A5A5A
MASK_POISON = 0x5A5A5A5A
PATTERN = r"[a-z]+|\s+|[^a-z\s]+"

_toks = {}


def _tok_of(name, vocab, specials, tmp_path_factory):
    if name not in _toks:
        from splintr_amd import Tokenizer
        path = tmp_path_factory.mktemp("dfa") / (name + ".tiktoken")
        path.write_bytes(vocabgen.tiktoken({b: i for i, b in vocab.items()}))
        _toks[name] = Tokenizer(str(path), PATTERN, {v.decode(): k for k, v in specials.items()})
    return _toks[name]


def _toy(name, tmp_path_factory):
    vocab, specials = cases.TOYS[name]()
    return _tok_of(name, vocab, specials, tmp_path_factory)


def _index(tok, table, n_states, n_words, *, off=0, keep=False):
    """spl_dfa_index_device into a poisoned buffer `off` bytes (a multiple of 4) behind a 16-byte boundary -> (rows uint32 [S, stride],
    some uint8 [S]); asserts that nothing around the index was written.  keep: also the device tensors (table, index view)."""
    import torch
    from splintr_amd import _ffi
    dev = torch.device("cuda", 0)
    stride = ref.stride(n_words)
    size = _ffi.SPL_DFA_INDEX_BYTES(n_states, n_words)
    assert size == n_states * (stride * 4 + 1)
    flat = torch.full((off + size + 64,), 0x5A, dtype=torch.uint8, device=dev)
    view = flat[off:off + size]
    assert view.data_ptr() % 16 == off % 16
    t_tab = torch.from_numpy(np.ascontiguousarray(table, dtype=np.uint8)).to(dev)
    rc = _ffi.lib().spl_dfa_index_device(tok.handle, t_tab.data_ptr(), n_states, n_words, view.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, _ffi.last_error()
    whole = flat.cpu().numpy()
    assert (whole[:off] == 0x5A).all() and (whole[off + size:] == 0x5A).all(), "written around the index"
    rows = whole[off:off + n_states * stride * 4].copy().view(np.uint32).reshape(n_states, stride)
    some = whole[off + n_states * stride * 4:off + size].copy()
    return (rows, some, t_tab, view) if keep else (rows, some)


def _call(tok, table, n_states, *, ids, state, lengths=None, flags=0, end_ids=(), n_words, in_place=False, mask_init=None, want_live=True, off16=0,
          index_off=0):
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
    _, _, t_tab, t_index = _index(tok, table, n_states, n_words, off=index_off, keep=True)
    t_ids = torch.from_numpy(ids.view(np.int32) if ids.dtype == np.uint32 else ids).to(dev)
    t_len = None if lengths is None else torch.from_numpy(np.ascontiguousarray(lengths, dtype=np.int32)).to(dev)
    rows = np.concatenate([np.asarray(state, dtype=np.uint64).reshape(B), np.full(1, WORD_POISON, dtype=np.uint64)])
    t_sin = torch.from_numpy(rows.view(np.int64)).to(dev)
    t_sout = t_sin if in_place else torch.full((B + 1,), WORD_POISON, dtype=torch.int64, device=dev)
    flat = torch.full(((B + 1) * n_words + 4,), MASK_POISON, dtype=torch.int32, device=dev)
    t_mask = flat[off16:off16 + (B + 1) * n_words].view(B + 1, n_words)
    assert t_mask.data_ptr() % 16 == 4 * off16
    init = None
    if mask_init is not None:
        init = np.asarray(mask_init, dtype=np.uint32)
        t_mask[:B] = torch.from_numpy(init.view(np.int32)).to(dev)
    t_live = torch.full((B + 1,), 0x5A, dtype=torch.uint8, device=dev)
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    si = _ffi.SplDfaIn(B, K, ptr(t_ids), ptr(t_len), t_sin.data_ptr(), t_tab.data_ptr(), t_index.data_ptr(), n_states)
    o = _ffi.SplDfaOpts(flags, n_words, end_ids)
    so = _ffi.SplDfaOut(t_sout.data_ptr(), t_mask.data_ptr(), t_live.data_ptr() if want_live else None)
    rc = _ffi.lib().spl_dfa_step_device(tok.handle, ctypes.byref(si), ctypes.byref(o), ctypes.byref(so), torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, _ffi.last_error()
    st = t_sout.cpu().numpy().view(np.uint64)
    whole = flat.cpu().numpy().view(np.uint32)
    mask = whole[off16:off16 + (B + 1) * n_words].reshape(B + 1, n_words)
    live = t_live.cpu().numpy()
    assert st[B] == WORD_POISON and (mask[B] == MASK_POISON).all() and live[B] == 0x5A, "written behind the rows"
    assert (whole[:off16] == MASK_POISON).all() and (whole[off16 + (B + 1) * n_words:] == MASK_POISON).all(), "written around the mask"
    if not want_live:
        assert (live == 0x5A).all()
    elif flags & ref.KEEP_FREE:
        keep = live[:B] == 0
        assert (mask[:B][keep] == (init[keep] if init is not None else MASK_POISON)).all(), "KEEP_FREE: a row that is not constrained was written"
    return dict(state=st[:B].copy(), mask=mask[:B].copy(), live=live[:B].copy())


def _runner(tok, **fixed):
    return lambda table, n_states, **kw: _call(tok, table, n_states, **dict(fixed, **kw))


def _indexer(tok, **fixed):
    return lambda table, n_states, n_words: _index(tok, table, n_states, n_words, **fixed)


# ---------------------------------------------------------------------------------------------- the toy enumerations
@pytest.mark.parametrize("name", sorted(cases.TOYS))
def test_toy_index(name, tmp_path_factory):
    tok = _toy(name, tmp_path_factory)
    cases.check_index(_indexer(tok), name, extra_words=(0, 1, 3))
    cases.check_index(_indexer(tok, off=4), name, sizes=(2, 65))


def test_toy_index_4096_states(tmp_path_factory):
    cases.check_index(_indexer(_toy("gaps", tmp_path_factory)), "gaps", sizes=(4096,))


@pytest.mark.parametrize("name", sorted(cases.TOYS))
def test_toy_against_guided_choice_and_every_probe_id(name, tmp_path_factory):
    tok = _toy(name, tmp_path_factory)
    cases.check_against_choice(_runner(tok), name, steps=6)
    cases.check_every_probe_id_from_every_state(_runner(tok), name)


def test_end_flags_layout_and_load(tmp_path_factory):
    tok = _toy("gaps", tmp_path_factory)
    run = _runner(tok)
    cases.check_end_ids(run)
    cases.check_flags(run)
    cases.check_layout_and_load(run, _indexer(tok))
    # a mask base 4 bytes behind a 16-byte boundary, an index base 8 bytes behind one: word accesses, whatever the row width; no live array
    cases.check_layout_and_load(_runner(tok, off16=1), _indexer(tok))
    cases.check_layout_and_load(_runner(tok, index_off=8), _indexer(tok, off=8))
    cases.check_end_ids(_runner(tok, off16=3))
    vocab, _, _ = cases.toy("gaps")
    tab = cases.alternation([b"ab"])
    r = _call(tok, ref.table_bytes(*tab), 3, ids=cases.NO_IDS(2), state=cases.words([ref.begin(0), ref.FREE]), end_ids=(4,), n_words=cases.min_words(vocab),
              want_live=False)
    assert r["state"].tolist() == [1 << 16, 0] and r["mask"].tolist() == [[0b101, 0], [0xFFFFFFFF] * 2]


# ---------------------------------------------------------------------------------------------- batch sizes, vocabulary sizes
@pytest.mark.parametrize("B", [0, 1, 63, 64, 65, 1025])
def test_batch_sizes(B, tmp_path_factory):
    tok = _toy("gaps", tmp_path_factory)
    vocab, specials, toks = cases.toy("gaps")
    nw = cases.min_words(vocab)
    tab = cases.compiled(cases.PROBE_PATTERNS["gaps"])
    S = ref.n_states(tab)
    rng = random.Random(B)
    start = [ref.begin(rng.randrange(S)) if b % 7 else ref.FREE for b in range(B)]
    ids = [[rng.choice(sorted(vocab))] for _ in range(B)]
    cases.expect(_runner(tok), toks, tab, cases.words(start), start, np.array(ids, dtype=np.int32).reshape(B, 1), nw, (4, 63))


def _sized_vocab(n):
    """n tokens, ids 0 .. n - 1: the strings of 1 .. 3 lower-case letters in id order by a fixed shuffle"""
    import itertools
    al = b"abcdefghijklmnopqrstuvwxyz"
    toks = [bytes(t) for k in (1, 2, 3) for t in itertools.product(al, repeat=k)][:n]
    random.Random(5).shuffle(toks)
    return dict(enumerate(toks))


@pytest.mark.parametrize("n", [4095, 4096, 4097, 4096 + 97])
def test_vocabulary_sizes_around_a_16_byte_access(n, tmp_path_factory):
    """4 095 and 4 096 ids: 128 words, the row ends at a 16-byte access; 4 097: 129 words, word accesses, stride 132; 4 193: 132 words.
    Every width also with three words more and with the mask base off its alignment; the index against the definition."""
    vocab = _sized_vocab(n)
    tok = _tok_of("sized%d" % n, vocab, {}, tmp_path_factory)
    toks = ref.ordinary(vocab)
    tab = cases.compiled(rb"ab[c-f]{0,2}(zz|q)?|[a-z]{3}")
    S = ref.n_states(tab)
    base = cases.min_words(vocab)
    start = [ref.begin(q) for q in range(S)] + [ref.FREE]
    for nw, off16 in ((base, 0), (base + 3, 0), (base, 1), (base + 4, 2)):
        end = (32 * nw - 1,)                                                  # (at 4 096 ids and 128 words an ordinary id)
        if off16 == 0:
            rows, some = _index(tok, ref.table_bytes(*tab), S, nw)
            want_rows, want_some = ref.index(toks, tab, nw)
            assert (rows == want_rows).all() and some.tolist() == want_some.tolist()
        r, states = cases.expect(_runner(tok, off16=off16), toks, tab, cases.words(start), start, cases.NO_IDS(len(start)), nw, end)
        ids = [[sorted(ref.allowed(toks, tab, st, end))[-1] if st[1] else 0] for st in states]
        cases.expect(_runner(tok, off16=off16), toks, tab, r["state"], states, ids, nw, end, in_place=True)


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals(tmp_path_factory):
    import torch
    from splintr_amd import _ffi, device as dv, dfa
    tok = _toy("gaps", tmp_path_factory)
    vocab, specials, _ = cases.toy("gaps")
    L = _ffi.lib()
    dev = torch.device("cuda", 0)
    nw = cases.min_words(vocab)
    d = dfa.compile_regex("ab|c")
    S = d.n_states
    ids = torch.zeros((2, 2), dtype=torch.int32, device=dev)
    lens = torch.ones(2, dtype=torch.int32, device=dev)
    st = torch.zeros(4, dtype=torch.int64, device=dev)
    st2 = torch.zeros(4, dtype=torch.int64, device=dev)
    mask = torch.zeros((2, nw), dtype=torch.int32, device=dev)
    live = torch.zeros(16, dtype=torch.uint8, device=dev)
    tab = dv.dfa_table(d, dev)
    index = dv.dfa_index_device(tok, tab, S, n_words=nw)
    assert tab.shape == (S * 513,) and index.shape == (_ffi.SPL_DFA_INDEX_BYTES(S, nw),)

    def go(si, o, so, word):
        assert L.spl_dfa_step_device(tok.handle, ctypes.byref(si) if si else None, ctypes.byref(o) if o else None, ctypes.byref(so) if so else None,
                                     None) == -1, word
        assert word in _ffi.last_error(), (word, _ffi.last_error())

    I = lambda **kw: _ffi.SplDfaIn(2, 2, kw.get("ids", ids.data_ptr()), kw.get("lens", lens.data_ptr()), kw.get("state", st.data_ptr()),
                                   kw.get("table", tab.data_ptr()), kw.get("index", index.data_ptr()), kw.get("n_states", S))
    P = lambda flags=0, n_words=nw, end=(4,): _ffi.SplDfaOpts(flags, n_words, end)
    O = lambda **kw: _ffi.SplDfaOut(kw.get("state", st2.data_ptr()), kw.get("mask", mask.data_ptr()), kw.get("live", live.data_ptr()))
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
    go(I(), P(n_words=nw - 1), O(), "n_words is too small")
    go(I(), P(n_words=(1 << 26) + 1), O(), "n_words is above 2^26")
    go(I(), P(1), O(), "unknown flag bit")
    go(I(), P(8), O(), "unknown flag bit")
    go(I(), P(1 << 31), O(), "unknown flag bit")
    o = P()
    o.n_end = 9
    go(I(), o, O(), "n_end is above SPL_DFA_MAX_END")
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
    big = _ffi.SplDfaIn((1 << 31), 0, None, None, st.data_ptr(), tab.data_ptr(), index.data_ptr(), S)
    go(big, P(), O(), "n_seqs >= 2^31")
    # the index call
    def gi(word, table=tab.data_ptr(), n_states=S, n_words=nw, out=index.data_ptr()):
        assert L.spl_dfa_index_device(tok.handle, table, n_states, n_words, out, None) == -1, word
        assert word in _ffi.last_error(), (word, _ffi.last_error())
    gi("d_table is null", table=None)
    gi("d_index is null", out=None)
    gi("n_states is 0", n_states=0)
    gi("n_states is 4097", n_states=4097)
    gi("n_words is too small", n_words=nw - 1)
    gi("n_words is above 2^26", n_words=(1 << 26) + 1)
    gi("not 2-byte aligned", table=tab.data_ptr() + 1)
    gi("not 4-byte aligned", out=index.data_ptr() + 2)
    gi("coincides with d_table", out=tab.data_ptr())
    # state out with state in is the one overlap allowed
    assert L.spl_dfa_step_device(tok.handle, ctypes.byref(I()), ctypes.byref(P()), ctypes.byref(O(state=st.data_ptr())), None) == 0
    torch.cuda.synchronize()
    # the Python layer: dtypes, shapes, sizes
    s2 = st[:2].contiguous()
    with pytest.raises(ValueError, match="int32 or int64"):
        dv.dfa_step_device(tok, ids.to(torch.int16), None, s2, tab, index, end_ids=[4])
    with pytest.raises(ValueError, match="END ids are needed"):
        dv.dfa_step_device(tok, ids, None, s2, tab, index, end_ids=[])
    with pytest.raises(ValueError, match="END ids are needed"):
        dv.dfa_step_device(tok, ids, None, s2, tab, index, end_ids=list(range(9)))
    with pytest.raises(ValueError, match="at or above 32"):
        dv.dfa_step_device(tok, ids, None, s2, tab, index, end_ids=[32 * nw], n_words=nw)
    with pytest.raises(ValueError, match="index must be"):
        dv.dfa_step_device(tok, ids, None, s2, tab, index, end_ids=[4], n_words=nw + 4)
    with pytest.raises(ValueError, match="keep_free needs"):
        dv.dfa_step_device(tok, ids, None, s2, tab, index, end_ids=[4], keep_free=True)
    with pytest.raises(ValueError, match=r"n_states \* 513"):
        dv.dfa_step_device(tok, ids, None, s2, tab[:100], index, end_ids=[4])
    with pytest.raises(ValueError, match=r"shape \[batch\]"):
        dv.dfa_step_device(tok, ids, None, st[:3].contiguous(), tab, index, end_ids=[4])
    with pytest.raises(ValueError, match="n_words is too small"):
        dv.dfa_index_device(tok, tab, S, n_words=nw - 1)
    with pytest.raises(ValueError, match="start 0 must be"):
        dv.dfa_state([4096])
    with pytest.raises(ValueError, match="n_states in 1 .. 4096"):
        dv.dfa_table((np.zeros((4097, 256), dtype=np.uint16), np.zeros(4097, dtype=np.uint8)))
    assert dv.dfa_state([0, None, 5], dev).cpu().tolist() == [1 << 16, 0, 5 | 1 << 16] and dv.dfa_n_words(tok) >= nw
    rows, some = dv.dfa_index_rows(index, S, nw)
    assert rows.shape == (S, ref.stride(nw)) and some.shape == (S,)
    out = dv.dfa_step_device(tok, None, None, dv.dfa_state([0, None], dev), tab, index, end_ids=[4], n_words=nw)
    assert out[0].cpu().tolist() == [1 << 16, 0] and out[2].cpu().tolist() == [1, 0]


# ---------------------------------------------------------------------------------------------- the shipped vocabularies, end to end
E2E = {
    "date": r"\d{4}-\d{2}-\d{2}",
    "uuid": r"[0-9a-f]{8}-[0-9a-f]{4}-[0-9a-f]{4}-[0-9a-f]{4}-[0-9a-f]{12}",
    "ipv4": r"((25[0-5]|2[0-4]\d|1\d\d|[1-9]?\d)\.){3}(25[0-5]|2[0-4]\d|1\d\d|[1-9]?\d)",
    "json": r'\{"id": [1-9]\d{0,3}, "ok": (true|false), "tags": \[("[a-z]{1,6}"(, "[a-z]{1,6}"){0,2})?\], "note": "[^"\\]{0,12}"\}',
}
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


def _np_row(d, q, ids, M, lens, stride):
    """brute force over every ordinary id at once: the row of state q"""
    S = d.n_states
    ext = np.concatenate([np.where(d.trans < S, d.trans, S).astype(np.int64), np.full((1, 256), S, dtype=np.int64)])      # (row S: dead stays dead)
    at = np.full(len(ids), q, dtype=np.int64)
    for j in range(M.shape[1]):
        on = np.flatnonzero((lens > j) & (at != S))
        if not len(on):
            break
        at[on] = ext[at[on], M[on, j]]
    ok = ids[at != S]
    row = np.zeros(stride, dtype=np.uint32)
    np.bitwise_or.at(row, ok >> 5, (np.uint32(1) << (ok & 31).astype(np.uint32)))
    return row


@pytest.mark.parametrize("pattern", sorted(E2E))
@pytest.mark.parametrize("name", ["cl100k_base", "o200k_base", "deepseek_v3"])
def test_shipped_vocabulary_end_to_end(name, pattern):
    import torch
    from splintr_amd import device as dv, dfa
    tok, ids, M, lens, by_id, special = _matrix(name)
    assert special is not None
    d = dfa.compile_regex(E2E[pattern])
    S, longest = d.n_states, d.longest()
    assert longest is not None                                                # a bounded pattern: a uniform sampler must terminate
    dev = torch.device("cuda", 0)
    nw = (tok.vocab_size + 31) // 32 + 3
    stride = ref.stride(nw)
    end = (special, 32 * nw - 1)
    table = dv.dfa_table(d, dev)
    index = dv.dfa_index_device(tok, table, S, n_words=nw)
    rows_t, some_t = dv.dfa_index_rows(index, S, nw)
    rows, some = rows_t.cpu().numpy().view(np.uint32), some_t.cpu().numpy()
    rng = random.Random(17)
    accepting = [q for q in range(S) if d.accept[q]]
    check = range(S) if pattern == "date" else sorted({0, *accepting, *rng.sample(range(S), 8)})
    for q in check:
        assert (rows[q] == _np_row(d, q, ids, M, lens, stride)).all(), (name, pattern, q)
    assert some.tolist() == (rows != 0).any(axis=1).astype(np.uint8).tolist()
    # B sequences draw uniformly from their masks until done
    B = 256
    state = dv.dfa_state([0] * B, dev)
    mask = torch.full((B, nw), -1, dtype=torch.int32, device=dev)
    live = torch.zeros(B, dtype=torch.uint8, device=dev)
    dv.dfa_step_device(tok, None, None, state, table, index, end_ids=end, mask=mask, state_out=state, live=live)
    first = mask[0].cpu().numpy().view(np.uint32)
    assert (first == rows[0][:nw]).all() and not d.accept[0]
    gen = torch.Generator(device=dev).manual_seed(5)
    shifts = torch.arange(32, device=dev, dtype=torch.int32)
    drawn = [b""] * B
    for step in range(longest + 1):
        alive = live.cpu().numpy().astype(bool)
        if not alive.any():
            break
        bits = ((mask.unsqueeze(-1) >> shifts) & 1).reshape(B, nw * 32).to(torch.float32)
        pick = torch.multinomial(bits, 1, generator=gen).flatten()          # the sampler: uniform over the row
        for b, t in enumerate(pick.cpu().tolist()):
            if alive[b]:
                drawn[b] += by_id.get(t, b"")                                # (an END id is no ordinary id here: it spells nothing)
        _, _, live = dv.dfa_step_device(tok, pick, live.to(torch.int32), state, table, index, end_ids=end, mask=mask, state_out=state)
    words = state.cpu().numpy()
    assert ((words >> 18) & 1).all() and not ((words >> 17) & 1).any() and not ((words >> 16) & 1).any(), "a sequence is not done after longest + 1 steps"
    assert all(d.accept[int(w) & 0xFFFF] for w in words)
    rx = re.compile(E2E[pattern].encode())
    for b in range(B):
        assert rx.fullmatch(drawn[b]) is not None, (name, pattern, b, drawn[b])
    assert (mask == -1).all().item()
    assert len(set(drawn)) > B // 8


# ---------------------------------------------------------------------------------------------- RegexGuide beside the streaming decode
def _uniform(mask, gen):
    import torch
    B, nw = mask.shape
    shifts = torch.arange(32, device=mask.device, dtype=torch.int32)
    bits = ((mask.unsqueeze(-1) >> shifts) & 1).reshape(B, nw * 32).to(torch.float32)
    return torch.multinomial(bits, 1, generator=gen).flatten()


def test_regex_guide_with_stream_decode_and_utf8_mask():
    import torch
    tok, ids, M, lens, by_id, special = _matrix("cl100k_base")
    pattern = r'[^"]{1,8}'
    B = 64
    guide = tok.regex_guide(B, pattern, end_ids=[special])
    dec = tok.device_streaming_decoder(B, skip_special_tokens=True)
    assert guide.begin() is guide.mask and guide.live.cpu().tolist() == [1] * B and guide.n_states == 9
    dev = guide.mask.device
    gen = torch.Generator(device=dev).manual_seed(11)
    texts, drawn = [""] * B, [b""] * B
    for step in range(10):
        if not guide.live.any().item():
            break
        before = guide.mask.clone()
        dec.allowed_mask(guide.mask, and_into=True)                             # the UTF-8 rows ANDed into the guide's
        assert ((guide.mask & ~before) == 0).all().item() and (guide.mask != 0).any(1).all().item()
        logits = torch.zeros((B, tok.vocab_size), dtype=torch.float32, device=dev)
        guide.apply(logits, live_only=True)
        pick = _uniform(guide.mask, gen)
        live = guide.live.cpu().numpy().astype(bool)
        for b, t in enumerate(pick.cpu().tolist()):
            if live[b]:
                assert logits[b, t].item() == 0.0
                drawn[b] += by_id.get(t, b"")
        lens_t = guide.live.to(torch.int32)                                     # sequences that are done draw nothing more
        out = dec.add_tokens(pick.to(torch.int32), lens_t)
        texts = [a + (o or "") for a, o in zip(texts, out)]
        guide.step(pick, lens_t)
        assert not dec.stalled.any().item(), "a sequence stalled"
    assert guide.done.all().item() and not guide.broken.any().item() and not guide.live.any().item()
    rx = re.compile(pattern.encode())
    for b in range(B):
        assert rx.fullmatch(drawn[b]) is not None, (b, drawn[b])
        got = texts[b].encode("utf-8")                                          # valid UTF-8 by construction of str; what the decoder let go
        assert drawn[b].startswith(got) and len(drawn[b]) - len(got) < 4, (b, drawn[b], got)
        drawn[b][:len(got)].decode("utf-8")
        assert not got or rx.fullmatch(got) is not None
    assert (guide.mask == -1).all().item()
    # rows begin again while the others keep their state; reset frees a row
    guide.begin([0], rows=[7])
    assert guide.live.cpu().tolist() == [int(b == 7) for b in range(B)] and guide.done.cpu().tolist() == [b != 7 for b in range(B)]
    guide.reset([7])
    assert guide.state.cpu().tolist()[7] == 0 and (guide.mask[7] == -1).all().item()


def test_stacked_patterns_with_select():
    import torch
    tok, ids, M, lens, by_id, special = _matrix("cl100k_base")
    pats = [r"\d{4}-\d{2}-\d{2}", r"(yes|no|maybe)!?"]
    B = 32
    guide = tok.regex_guide(B, pats, end_ids=[special])
    assert guide.starts == [0, 11] and guide.n_states == 11 + guide.dfas[1].n_states
    select = [b % 2 for b in range(B)]
    select[4] = select[5] = None
    guide.begin(select)
    assert guide.live.cpu().tolist() == [0 if s is None else 1 for s in select]
    dev = guide.mask.device
    gen = torch.Generator(device=dev).manual_seed(3)
    drawn = [b""] * B
    for step in range(12):
        live = guide.live.cpu().numpy().astype(bool)
        if not live.any():
            break
        pick = _uniform(guide.mask, gen)
        for b, t in enumerate(pick.cpu().tolist()):
            if live[b]:
                drawn[b] += by_id.get(t, b"")
        guide.step(pick, guide.live.to(torch.int32))
    done = guide.done.cpu().tolist()
    for b in range(B):
        if select[b] is None:
            assert not done[b] and guide.state.cpu().tolist()[b] == 0 and drawn[b] == b""
        else:
            assert done[b] and re.fullmatch(pats[select[b]].encode(), drawn[b]) is not None, (b, drawn[b])
    assert not guide.broken.any().item()
    with pytest.raises(ValueError, match="patterns are 0 .. 1"):
        guide.begin([2] * B)
