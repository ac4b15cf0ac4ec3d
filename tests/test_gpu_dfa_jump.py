"""GPU tests (-m gpu): spl_dfa_jump_index_device and spl_dfa_jump_device -- jump-forward for the regex guide, forced runs emitted as ids --
through the C ABI into guarded buffers against the definition of tests/jump_ref.py: the checks of tests/jump_cases.py over the toy
vocabularies, generated vocabularies of 4 095 and 4 193 ids, batch sizes around the kernels' edges, widths of the forced rows, mask and
index bases off their 16-byte alignment, every refusal; on the shipped vocabularies the jump index of the JSON, tool and date patterns
state by state against the definition and the tokenizer's own encode; RegexGuide.jump end to end with a uniform sampler and the draws
counted against the same loop without jump; the forced ids through DeviceStreamingDecoder; a stacked two-pattern batch."""
import ctypes
import random
import re

import numpy as np
import pytest

import dfa_ref as ref
import jump_cases as cases
import jump_ref as jref
import vocabgen

pytestmark = pytest.mark.gpu

WORD_POISON = 0x5A5A5A5A5A5A5A5A
MASK_POISON = 0x5A5A5A5A
PATTERN = r"[a-z]+|\s+|[^a-z\s]+"
JSON = r'\{"name": "[a-z]+", "age": [0-9]{1,3}\}'
TOOL = r"<tool>(get_weather|get_time)</tool>"
DATE = r"\d{4}-\d{2}-\d{2}"
SHIPPED = ["cl100k_base", "o200k_base", "deepseek_v3"]

_toks = {}
_shipped = {}


@pytest.fixture(scope="module", autouse=True)
def _release_the_tokenizers():
    """The tokenizers this module keeps (and the streams their encode and decode pipelines picked: hardware queues are few) go with the
    module, not with the process: what runs behind it finds the GPU's queues as this module found them."""
    yield
    import gc
    import torch
    _toks.clear()
    _shipped.clear()
    gc.collect()
    torch.cuda.synchronize()


def _tok_of(name, vocab, specials, tmp_path_factory):
    if name not in _toks:
        from splintr_amd import Tokenizer
        path = tmp_path_factory.mktemp("jump") / (name + ".tiktoken")
        path.write_bytes(vocabgen.tiktoken({b: i for i, b in vocab.items()}))
        _toks[name] = Tokenizer(str(path), PATTERN, {v.decode(): k for k, v in specials.items()})
    return _toks[name]


def _toy(name, tmp_path_factory):
    vocab, specials = cases.TOYS[name]()
    return _tok_of(name, vocab, specials, tmp_path_factory)


def _dev():
    import torch
    return torch.device("cuda", 0)


def _stream():
    import torch
    return torch.cuda.current_stream(_dev()).cuda_stream


def _jump_index(tok, table, n_states, *, off=0):
    """spl_dfa_jump_index_device into a poisoned buffer `off` bytes (a multiple of 4) behind a 16-byte boundary -> the index's bytes;
    asserts that nothing around the index was written."""
    import torch
    from splintr_amd import _ffi
    size = _ffi.SPL_DFA_JUMP_INDEX_BYTES(n_states)
    flat = torch.full((off + size + 64,), 0x5A, dtype=torch.uint8, device=_dev())
    view = flat[off:off + size]
    assert view.data_ptr() % 16 == off % 16
    t_tab = torch.from_numpy(np.ascontiguousarray(table, dtype=np.uint8)).to(_dev())
    rc = _ffi.lib().spl_dfa_jump_index_device(tok.handle, t_tab.data_ptr(), n_states, view.data_ptr(), _stream())
    assert rc == 0, _ffi.last_error()
    whole = flat.cpu().numpy()
    assert (whole[:off] == 0x5A).all() and (whole[off + size:] == 0x5A).all(), "written around the jump index"
    return whole[off:off + size].copy()


def _runs(tok):
    def runs(table, n_states):
        _, _, run_len, run = jref.index_parts(_jump_index(tok, table, n_states), n_states)
        return run, run_len
    return runs


def _call(tok, table, n_states, *, ids, state, jump_index=None, row_len_out=16, lengths=None, flags=0, end_ids=(), n_words, in_place=False, mask_init=None,
          off16=0, index_off=0, jump_off=0):
    """One call through the C ABI -- spl_dfa_jump_device, or spl_dfa_step_device with jump_index None -- the index built by the kernels in
    front of it, with poisoned outputs and a spare row behind each -> dict of numpy arrays; asserts that nothing behind or around the rows
    was written.  off16: words the mask base lies behind a 16-byte boundary; index_off / jump_off: bytes the index / the jump index lies
    behind one."""
    import torch
    from splintr_amd import _ffi
    dev = _dev()
    ids = np.ascontiguousarray(ids)
    B, K = ids.shape
    if ids.dtype == np.int64:
        flags |= ref.I64
    t_tab = torch.from_numpy(np.ascontiguousarray(table, dtype=np.uint8)).to(dev)
    isize = _ffi.SPL_DFA_INDEX_BYTES(n_states, n_words)
    t_index = torch.full((index_off + isize + 16,), 0x5A, dtype=torch.uint8, device=dev)[index_off:index_off + isize]
    assert _ffi.lib().spl_dfa_index_device(tok.handle, t_tab.data_ptr(), n_states, n_words, t_index.data_ptr(), _stream()) == 0, _ffi.last_error()
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
    so = _ffi.SplDfaOut(t_sout.data_ptr(), t_mask.data_ptr(), t_live.data_ptr())
    if jump_index is None:
        rc = _ffi.lib().spl_dfa_step_device(tok.handle, ctypes.byref(si), ctypes.byref(o), ctypes.byref(so), _stream())
    else:
        jump_index = np.ascontiguousarray(jump_index, dtype=np.uint8)
        assert jump_index.size == _ffi.SPL_DFA_JUMP_INDEX_BYTES(n_states)
        t_jflat = torch.full((jump_off + jump_index.size + 16,), 0x5A, dtype=torch.uint8, device=dev)
        t_jump = t_jflat[jump_off:jump_off + jump_index.size]
        t_jump.copy_(torch.from_numpy(jump_index))
        t_forced = torch.full((B + 1, row_len_out), cases.FORCED_POISON, dtype=torch.int32, device=dev)
        t_flen = torch.full((B + 1,), cases.FORCED_POISON, dtype=torch.int32, device=dev)
        jo = _ffi.SplDfaJumpOut(row_len_out, t_jump.data_ptr(), t_forced.data_ptr(), t_flen.data_ptr())
        rc = _ffi.lib().spl_dfa_jump_device(tok.handle, ctypes.byref(si), ctypes.byref(o), ctypes.byref(so), ctypes.byref(jo), _stream())
    assert rc == 0, _ffi.last_error()
    st = t_sout.cpu().numpy().view(np.uint64)
    whole = flat.cpu().numpy().view(np.uint32)
    mask = whole[off16:off16 + (B + 1) * n_words].reshape(B + 1, n_words)
    live = t_live.cpu().numpy()
    assert st[B] == WORD_POISON and (mask[B] == MASK_POISON).all() and live[B] == 0x5A, "written behind the rows"
    assert (whole[:off16] == MASK_POISON).all() and (whole[off16 + (B + 1) * n_words:] == MASK_POISON).all(), "written around the mask"
    if flags & ref.KEEP_FREE:
        keep = live[:B] == 0
        assert (mask[:B][keep] == (init[keep] if init is not None else MASK_POISON)).all(), "KEEP_FREE: a row that is not constrained was written"
    out = dict(state=st[:B].copy(), mask=mask[:B].copy(), live=live[:B].copy())
    if jump_index is not None:
        forced, flen = t_forced.cpu().numpy(), t_flen.cpu().numpy()
        assert (forced[B] == cases.FORCED_POISON).all() and flen[B] == cases.FORCED_POISON, "written behind the forced rows"
        assert (t_jflat.cpu().numpy()[jump_off:jump_off + jump_index.size] == jump_index).all(), "the step wrote into the jump index"
        out.update(forced=forced[:B].copy(), forced_len=flen[:B].copy())
    return out


def _runner(tok, **fixed):
    return lambda table, n_states, **kw: _call(tok, table, n_states, **dict(fixed, **kw))


# ---------------------------------------------------------------------------------------------- the toy enumerations
@pytest.mark.parametrize("name", sorted(cases.TOYS))
def test_toy_runs(name, tmp_path_factory):
    cases.check_runs(_runs(_toy(name, tmp_path_factory)), name)


def test_toy_runs_4096_states_and_an_index_off_its_alignment(tmp_path_factory):
    tok = _toy("gaps", tmp_path_factory)
    cases.check_runs(_runs(tok), "gaps", sizes=(4096,))
    tab = cases.forced_automaton(65, cases.dfa_cases.alphabet_of(cases.toy("gaps")[2]), 5)       # (odd: run[] lies 2 bytes off a word)
    for off in (4, 8, 12):
        p = jref.index_parts(_jump_index(tok, ref.table_bytes(*tab), 65, off=off), 65)
        want, want_len = jref.run_arrays(tab)
        assert (p[3] == want).all() and p[2].tolist() == want_len.tolist()


@pytest.mark.parametrize("name", sorted(cases.TOYS))
def test_toy_jump_against_the_definition(name, tmp_path_factory):
    cases.check_jump(_runner(_toy(name, tmp_path_factory)), name, row_lens=(1, 3, 16, 64))


def test_adversarial_tables_keep_free_layouts_and_the_zero_index(tmp_path_factory):
    tok = _toy("gaps", tmp_path_factory)
    run = _runner(tok)
    cases.check_adversarial(run)
    cases.check_keep_free_and_layouts(run)
    cases.check_zero_index_is_the_step(run, run)                               # (the same runner without a jump index: spl_dfa_step_device)
    # a mask base 4 bytes behind a 16-byte boundary, an index base 8 and a jump index base 4 bytes behind one
    cases.check_keep_free_and_layouts(_runner(tok, off16=1))
    cases.check_keep_free_and_layouts(_runner(tok, index_off=8, jump_off=4))
    cases.check_adversarial(_runner(tok, off16=3, jump_off=12))


# ---------------------------------------------------------------------------------------------- batch sizes, vocabulary sizes
@pytest.mark.parametrize("B", [0, 1, 63, 64, 65, 1025])
def test_batch_sizes(B, tmp_path_factory):
    tok = _toy("gaps", tmp_path_factory)
    vocab, specials, toks = cases.toy("gaps")
    nw = cases.min_words(vocab)
    tab = cases.compiled(cases.JUMP_PATTERNS["gaps"])
    S = ref.n_states(tab)
    jidx = cases.reference_index("gaps", tab)
    rng = random.Random(B)
    start = [ref.begin(rng.randrange(S)) if b % 7 else ref.FREE for b in range(B)]
    ids = [[rng.choice(sorted(vocab))] for _ in range(B)]
    lens = np.array([b % 2 for b in range(B)], dtype=np.int32)
    cases.expect(_runner(tok), toks, tab, cases.words(start), start, np.array(ids, dtype=np.int32).reshape(B, 1), jidx, 3, nw, (4, 63), lengths=lens)


def _sized_vocab(n):
    """n tokens, ids 0 .. n - 1: the strings of 1 .. 3 lower-case letters in id order by a fixed shuffle"""
    import itertools
    al = b"abcdefghijklmnopqrstuvwxyz"
    toks = [bytes(t) for k in (1, 2, 3) for t in itertools.product(al, repeat=k)][:n]
    random.Random(5).shuffle(toks)
    return dict(enumerate(toks))


@pytest.mark.parametrize("n", [4095, 4096 + 97])
def test_generated_vocabularies(n, tmp_path_factory):
    """4 095 ids: 128 words, 16-byte accesses; 4 193: 132 words.  The jump index the kernels build: the runs are the definition's, the ids
    the tokenizer's own encode of each run; then the jump step with that index from every state, at the minimum width and three words more."""
    vocab = _sized_vocab(n)
    tok = _tok_of("sized%d" % n, vocab, {}, tmp_path_factory)
    toks = ref.ordinary(vocab)
    tab = cases.compiled(rb"abcab[c-f]{1,2}(zzzz|q)xyzzy(k|pqrst)")
    S = ref.n_states(tab)
    jidx = _jump_index(tok, ref.table_bytes(*tab), S)
    j_ids, j_n, run_len, run = jref.index_parts(jidx, S)
    want, want_len = jref.run_arrays(tab)
    assert (run == want).all() and run_len.tolist() == want_len.tolist() and int((want_len > 2).sum()) >= 4
    for q in range(S):
        text = bytes(run[q, :run_len[q]])
        assert j_ids[q, :j_n[q]].tolist() == tok.encode(text.decode()) and (j_ids[q, j_n[q]:] == 0).all(), q
        assert b"".join(vocab[int(i)] for i in j_ids[q, :j_n[q]]) == text
    base = cases.min_words(vocab)
    start = [ref.begin(q) for q in range(S)] + [ref.FREE]
    for nw, off16 in ((base, 0), (base + 3, 1)):
        for K in (1, 16):
            _, after, out = cases.expect(_runner(tok, off16=off16), toks, tab, cases.words(start), start, cases.NO_IDS(len(start)), jidx, K, nw, (32 * nw - 1,))
            if K == 16:                                                       # the whole run was emitted: no state is still forced
                assert all(b"".join(vocab[i] for i in o) == bytes(run[q, :run_len[q]]) for q, o in enumerate(out[:S]))
                assert all(jref.force(tab, s[0]) is None for s in after[:S] if s[1])


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals(tmp_path_factory):
    """Every refusal the two calls add -- with addresses no device call could follow: were the device touched first, these calls could not
    return SPL_EINVAL with these messages -- what the plain step refuses under this call's name, and the Python layer's ValueErrors."""
    import torch
    from splintr_amd import _ffi, device as dv, dfa
    tok = _toy("gaps", tmp_path_factory)
    vocab, specials, _ = cases.toy("gaps")
    L = _ffi.lib()
    h = tok.handle
    nw = cases.min_words(vocab)
    A = 0x1000

    def call(i=None, o=None, out=None, jo=None):
        i = i or _ffi.SplDfaIn(1, 1, A, None, A + 64, A + 128, A + 256, 2)
        o = o or _ffi.SplDfaOpts(0, nw, (7,))
        out = out or _ffi.SplDfaOut(A + 512, A + 1024, None)
        jo = jo or _ffi.SplDfaJumpOut(16, A + 2048, A + 4096, A + 8192)
        rc = L.spl_dfa_jump_device(h, ctypes.byref(i), ctypes.byref(o), ctypes.byref(out), ctypes.byref(jo), None)
        return rc, L.spl_last_error()

    J = _ffi.SplDfaJumpOut
    for jo, msg in ((J(0, A, A + 64, A + 128), b"row_len_out is 0"), (J(65, A, A + 64, A + 128), b"row_len_out is 65"),
                    (J(16, None, A + 64, A + 128), b"d_jump_index is null"), (J(16, A, None, A + 128), b"d_forced_ids is null"),
                    (J(16, A, A + 64, None), b"d_forced_len is null"), (J(16, A + 2, A + 64, A + 128), b"not 4-byte aligned"),
                    (J(16, A, A + 65, A + 128), b"not 4-byte aligned"), (J(16, A, A + 64, A + 130), b"not 4-byte aligned"),
                    (J(16, A + 2048, A + 512, A + 8192), b"d_forced_ids coincides"), (J(16, A + 2048, A + 4096, A + 1024), b"d_forced_len coincides"),
                    (J(16, A + 2048, A + 4096, A + 4096), b"coincides"), (J(16, A + 1024, A + 4096, A + 8192), b"d_jump_index coincides")):
        rc, err = call(jo=jo)
        assert rc == -1 and b"spl_dfa_jump_device" in err and msg in err, (msg, err)
    short = J(16, A + 2048, A + 4096, A + 8192)
    short.struct_size = 8
    rc, err = call(jo=short)
    assert rc == -1 and b"spl_dfa_jump_out" in err
    I = _ffi.SplDfaIn
    for kw, msg in ((dict(o=_ffi.SplDfaOpts(0, nw, ())), b"n_end is 0"), (dict(o=_ffi.SplDfaOpts(64, nw, (7,))), b"flag"),
                    (dict(i=I(1, 1, A, None, A + 64, A + 128, A + 256, 0)), b"n_states is 0"), (dict(o=_ffi.SplDfaOpts(0, nw - 1, (7,))), b"n_words is too small"),
                    (dict(i=I(1, 1, A, None, None, A + 128, A + 256, 2)), b"d_state_in is null"), (dict(out=_ffi.SplDfaOut(A + 512, None, None)), b"d_mask is null"),
                    (dict(i=I(1, 1, A, None, A + 64, None, A + 256, 2)), b"d_table is null"), (dict(i=I(1 << 31, 0, None, None, A + 64, A + 128, A + 256, 2)), b"n_seqs >= 2^31"),
                    (dict(out=_ffi.SplDfaOut(A + 512, A + 64, None)), b"coincides with an input")):
        rc, err = call(**kw)
        assert rc == -1 and b"spl_dfa_jump_device" in err and msg in err, (msg, err)
    assert L.spl_dfa_jump_device(h, None, None, None, None, None) == -1 and b"spl_dfa_jump_device" in L.spl_last_error()
    assert L.spl_dfa_jump_device(h, ctypes.byref(I(1, 1, A, None, A + 64, A + 128, A + 256, 2)), None, None, ctypes.byref(J(16, A + 2048, A + 4096, A + 8192)), None) == -1
    for args, msg in (((None, 2, A), b"d_table is null"), ((A + 1, 2, A), b"not 2-byte aligned"), ((A, 0, A), b"n_states is 0"), ((A, 4097, A), b"n_states is 4097"),
                      ((A, 2, None), b"d_jump_index is null"), ((A, 2, A + 2), b"not 4-byte aligned"), ((A, 2, A), b"coincides with d_table")):
        assert L.spl_dfa_jump_index_device(h, args[0], args[1], args[2], None) == -1
        assert b"spl_dfa_jump_index_device" in L.spl_last_error() and msg in L.spl_last_error(), (msg, L.spl_last_error())
    # the Python layer
    dev = _dev()
    d = dfa.compile_regex("abc(ab|c)")
    S = d.n_states
    tab = dv.dfa_table(d, dev)
    index = dv.dfa_index_device(tok, tab, S, n_words=nw)
    jidx = dv.dfa_jump_index_device(tok, tab, S)
    assert jidx.shape == (S * 322,) and [v.shape for v in dv.dfa_jump_index_views(jidx, S)] == [(S, 64), (S,), (S,), (S, 64)]
    ids = torch.zeros((2, 1), dtype=torch.int32, device=dev)
    st = dv.dfa_state([0, None], dev)
    go = lambda **kw: dv.dfa_jump_device(tok, kw.pop("ids", ids), None, st, tab, index, kw.pop("jump_index", jidx), end_ids=[4], n_words=nw, **kw)
    with pytest.raises(ValueError, match="jump_index must be"):
        go(jump_index=jidx[:-2])
    with pytest.raises(ValueError, match="jump_index must be"):
        go(jump_index=jidx.to(torch.int8))
    with pytest.raises(ValueError, match="row_len_out"):
        go(row_len_out=0)
    with pytest.raises(ValueError, match="row_len_out"):
        go(row_len_out=65)
    with pytest.raises(ValueError, match="forced_ids must be"):
        go(forced_ids=torch.zeros((3, 4), dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="forced_ids must be"):
        go(forced_ids=torch.zeros((2, 4), dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="row_len_out"):
        go(forced_ids=torch.zeros((2, 65), dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="forced_len must be"):
        go(forced_len=torch.zeros(3, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="int32 or int64"):
        go(ids=ids.to(torch.int16))
    with pytest.raises(ValueError, match="out must be"):
        dv.dfa_jump_index_device(tok, tab, S, out=torch.zeros(5, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="jump index must be"):
        dv.dfa_jump_index_views(jidx[:-1], S)
    with pytest.raises(ValueError, match="jump_ids must be"):
        tok.regex_guide(2, "ab", end_ids=[4], jump=True, jump_ids=65)
    plain = tok.regex_guide(2, "ab", end_ids=[4])
    with pytest.raises(ValueError, match="without jump=True"):
        plain.jump()
    with pytest.raises(ValueError, match="without jump=True"):
        plain.forced_text(0)
    so, mask, live, forced, flen = go(ids=None)
    assert forced.shape == (2, 16) and live.cpu().tolist() == [1, 0] and so.cpu().tolist()[1] == 0 and flen.cpu().tolist()[1] == 0
    emitted = b"".join(vocab[i] for i in forced[0, :int(flen[0])].cpu().tolist())
    assert b"abc".startswith(emitted) and ref.walk((d.trans, d.accept), 0, emitted) == int(so[0]) & 0xFFFF      # whatever was emitted walks
    empty = dv.dfa_jump_device(tok, None, None, dv.dfa_state([], dev), tab, index, jidx, end_ids=[4], n_words=nw)
    assert [tuple(t.shape) for t in empty] == [(0,), (0, nw), (0,), (0, 16), (0,)]


# ---------------------------------------------------------------------------------------------- the shipped vocabularies

def _shipped_tok(name):
    if name not in _shipped:
        from splintr_amd import Tokenizer, _ffi
        tok = Tokenizer.from_pretrained(name)
        p, n = ctypes.c_void_p(), ctypes.c_uint32()
        by_id, special = {}, None
        for i in range(tok.vocab_size):
            kind = _ffi.lib().spl_token_bytes(tok.handle, i, ctypes.byref(p), ctypes.byref(n))
            if kind in (1, 2) and n.value:
                by_id[i] = ctypes.string_at(p, n.value)
            elif kind == 3:
                special = i
        assert special is not None
        _shipped[name] = (tok, special, by_id)
    return _shipped[name][:2]


@pytest.mark.parametrize("name", SHIPPED)
def test_shipped_vocabulary_jump_index(name):
    """For the JSON, tool and date patterns and every state q: run and run_len are the definition's; ids[q][:n_ids[q]] is
    Tokenizer.encode(run(q)) and decodes back to the run; walking those ids from q with the existing dfa_step_device arrives at the state
    jump arrives at, with the same mask."""
    import torch
    from splintr_amd import device as dv, dfa
    tok, special = _shipped_tok(name)
    dev = _dev()
    for pattern in (JSON, TOOL, DATE):
        d = dfa.compile_regex(pattern)
        S = d.n_states
        tab = (d.trans, d.accept)
        table = dv.dfa_table(d, dev)
        index = dv.dfa_index_device(tok, table, S)
        jidx = dv.dfa_jump_index_device(tok, table, S)
        ids_t, n_t, len_t, run_t = dv.dfa_jump_index_views(jidx, S)
        j_ids, j_n, run_len, run = ids_t.cpu().numpy(), n_t.cpu().numpy(), len_t.cpu().numpy(), run_t.cpu().numpy()
        want, want_len = jref.run_arrays(tab)
        assert (run == want).all() and run_len.tolist() == want_len.tolist(), (name, pattern)
        assert (j_n > 0).tolist() == (run_len > 0).tolist()
        for q in range(S):
            text = bytes(run[q, :run_len[q]])
            got = j_ids[q, :j_n[q]].tolist()
            assert got == tok.encode(text.decode()) and (j_ids[q, j_n[q]:] == 0).all(), (name, pattern, q)
            assert tok.decode_bytes(got) == text
        if pattern == DATE:
            assert sorted(bytes(run[q, :run_len[q]]) for q in range(S) if run_len[q]) == [b"-", b"-"]
        # from every state: the jump, and the plain step fed the same ids
        st = dv.dfa_state(list(range(S)), dev)
        s_j, m_j, l_j, forced, flen = dv.dfa_jump_device(tok, None, None, st, table, index, jidx, end_ids=[special], row_len_out=64)
        assert flen.cpu().tolist() == j_n.tolist() and all(forced[q, :j_n[q]].cpu().tolist() == j_ids[q, :j_n[q]].tolist() for q in range(S))
        s_s, m_s, l_s = dv.dfa_step_device(tok, forced, flen, st, table, index, end_ids=[special])
        assert torch.equal(s_j, s_s) and torch.equal(m_j, m_s) and torch.equal(l_j, l_s), (name, pattern)
        arrived = (s_j.cpu().numpy() & 0xFFFF).tolist()
        assert all(arrived[q] == ref.walk(tab, q, bytes(run[q, :run_len[q]])) for q in range(S))


def _uniform(mask, gen, only=None):
    import torch
    B, nw = mask.shape
    shifts = torch.arange(32, device=mask.device, dtype=torch.int32)
    bits = ((mask.unsqueeze(-1) >> shifts) & 1).reshape(B, nw * 32).to(torch.float32)
    if only is not None:
        narrowed = bits * only
        keep = narrowed.sum(1, keepdim=True) > 0                              # (a row the restriction would empty keeps its whole mask)
        bits = torch.where(keep, narrowed, bits)
    return torch.multinomial(bits, 1, generator=gen).flatten()


def _generate(name, pattern, B, jump, seed, leave_after=3, max_steps=48):
    """begin(), then a loop of jump() (or step()) and a uniform draw from the mask until every sequence is done.  The name of the JSON
    pattern has no upper bound, so once a sequence has drawn `leave_after` ids in states that are not forced, its draw is uniform over
    the allowed ids that hold no lower-case letter (still a draw from its mask; a row that would be empty keeps the whole mask) -- the
    same rule with and without jump.  -> (texts, per sequence the states in which it drew an ordinary id, END draws per sequence, the
    guide)"""
    import torch
    from splintr_amd import dfa
    tok, special = _shipped_tok(name)
    by_id = _shipped[name][2]
    d = dfa.compile_regex(pattern)
    forced_state = [jref.force((d.trans, d.accept), q) is not None for q in range(d.n_states)]
    guide = tok.regex_guide(B, pattern, end_ids=[special], jump=jump)
    dev = guide.mask.device
    nw = guide.n_words
    lower = re.compile(rb"[a-z]")
    no_letters = torch.zeros(nw * 32, dtype=torch.float32, device=dev)
    no_letters[torch.tensor([i for i, b in by_id.items() if not lower.search(b)] + [special], device=dev)] = 1.0
    gen = torch.Generator(device=dev).manual_seed(seed)
    texts, drew_in, ends = [b""] * B, [[] for _ in range(B)], [0] * B

    def take(forced, flen):
        for b, (row, m) in enumerate(zip(forced.cpu().tolist(), flen.cpu().tolist())):
            texts[b] += b"".join(by_id[t] for t in row[:m])

    guide.begin()
    if jump:
        take(*guide.jump())
    for step in range(max_steps):
        live = guide.live.cpu().numpy().astype(bool)
        if not live.any():
            break
        leave = torch.tensor([[1.0 if sum(not forced_state[q] for q in qs) >= leave_after else 0.0] for qs in drew_in], device=dev)
        pick = _uniform(guide.mask, gen, only=leave * no_letters + (1.0 - leave))
        q = guide.q.cpu().tolist()
        for b, t in enumerate(pick.cpu().tolist()):
            if live[b]:
                if t == special:
                    ends[b] += 1
                else:
                    drew_in[b].append(q[b])
                    texts[b] += by_id[t]
        lens = guide.live.to(torch.int32)
        if jump:
            take(*guide.jump(pick, lens))
        else:
            guide.step(pick, lens)
    return texts, drew_in, ends, guide, forced_state


@pytest.mark.parametrize("name", SHIPPED)
def test_end_to_end_draws_with_and_without_jump(name):
    """256 sequences of the JSON pattern.  With jump every finished text is a fullmatch and a sequence draws ONLY where the automaton
    leaves a choice -- the name's and the age's tokens -- plus one END: never in a forced state.  The same loop without jump also
    finishes with fullmatches, but every sequence draws in forced states (its first state is one), and the loop needs strictly more
    draws: the draws in states that are not forced follow the same rule in both loops, the forced ones come on top."""
    B = 256
    rx = re.compile(JSON.encode())
    texts, drew_in, ends, guide, forced_state = _generate(name, JSON, B, True, 5)
    assert guide.done.all().item() and not guide.broken.any().item()
    assert all(rx.fullmatch(t) for t in texts), [t for t in texts if not rx.fullmatch(t)][:3]
    assert ends == [1] * B
    assert not any(forced_state[q] for qs in drew_in for q in qs), "a draw in a forced state"
    assert len(set(texts)) > B // 8
    with_jump = sum(len(qs) for qs in drew_in) + sum(ends)
    texts0, drew0, ends0, guide0, _ = _generate(name, JSON, B, False, 5)
    assert guide0.done.all().item() and all(rx.fullmatch(t) for t in texts0) and ends0 == [1] * B
    assert all(any(forced_state[q] for q in qs) for qs in drew0)
    without = sum(len(qs) for qs in drew0) + sum(ends0)
    print("%s: draws with jump %d, without %d, of those in forced states %d (B = %d)" %
          (name, with_jump, without, sum(sum(forced_state[q] for q in qs) for qs in drew0), B))
    assert without > with_jump


def test_literal_pattern_finishes_with_no_draw_but_end():
    texts, drew_in, ends, guide, _ = _generate("cl100k_base", "hello world", 8, True, 3)
    assert texts == [b"hello world"] * 8 and drew_in == [[]] * 8 and ends == [1] * 8 and guide.done.all().item()
    assert guide.forced_text(0) == b"hello world"


def test_forced_ids_through_the_streaming_decoder():
    """forced_ids and forced_len have the [B, K] + lengths form DeviceStreamingDecoder.add_tokens takes: the run's text comes out."""
    import torch
    tok, special = _shipped_tok("cl100k_base")
    B = 4
    guide = tok.regex_guide(B, TOOL, end_ids=[special], jump=True, jump_ids=16)
    dec = tok.device_streaming_decoder(B)
    guide.begin([0, 0, None, 0])
    forced, n = guide.jump()
    assert n.cpu().tolist()[2] == 0 and guide.forced_text(0) == b"<tool>get_"
    out = dec.add_tokens(forced, n)
    assert [o or "" for o in out] == ["<tool>get_", "<tool>get_", "", "<tool>get_"]
    # "w" is drawn; the rest of the answer is forced
    w = tok.encode("w")
    assert len(w) == 1
    pick = torch.tensor([w[0]] * B, dtype=torch.int32, device=guide.mask.device)
    forced, n = guide.jump(pick, guide.live.to(torch.int32))
    out = dec.add_tokens(forced, n)
    assert [o or "" for o in out] == ["eather</tool>", "eather</tool>", "", "eather</tool>"]
    assert forced[0, :int(n[0])].cpu().tolist() == tok.encode("eather</tool>")
    assert guide.live.cpu().tolist() == [1, 1, 0, 1] and (guide.q.cpu()[[0, 1, 3]] == guide.q.cpu()[0]).all()
    guide.jump(torch.tensor([special] * B, dtype=torch.int32, device=guide.mask.device), guide.live.to(torch.int32))
    assert guide.done.cpu().tolist() == [True, True, False, True] and guide.forced_len.cpu().tolist() == [0] * B


def test_stacked_patterns_and_a_narrow_row():
    """Two patterns in one table, a sequence that runs free; jump_ids 2: a run of more ids is continued by the next calls."""
    import torch
    tok, special = _shipped_tok("cl100k_base")
    pats = [TOOL, r"answer: (yes|no)"]
    B = 6
    guide = tok.regex_guide(B, pats, end_ids=[special], jump=True, jump_ids=2)
    select = [0, 1, None, 1, 0, 1]
    guide.begin(select)
    texts = [b""] * B
    want_first = [b"<tool>get_", b"answer: ", b"", b"answer: ", b"<tool>get_", b"answer: "]
    for _ in range(8):
        forced, n = guide.jump()
        if not n.any().item():
            break
        assert (n <= 2).all().item()
        for b in range(B):
            texts[b] += tok.decode_bytes(forced[b, :int(n[b])].cpu().tolist())
    assert texts == want_first
    assert [guide.forced_text(s) for s in guide.starts] == [b"<tool>get_", b"answer: "]
    assert guide.live.cpu().tolist() == [0 if s is None else 1 for s in select] and guide.state.cpu().tolist()[2] == 0
    assert (guide.mask[2] == -1).all().item() and not guide.broken.any().item()


def test_a_guide_without_jump_is_untouched():
    tok, special = _shipped_tok("cl100k_base")
    plain = tok.regex_guide(3, DATE, end_ids=[special])
    assert plain.jump_index is None and plain.forced_ids is None and plain.forced_len is None
    with_jump = tok.regex_guide(3, DATE, end_ids=[special], jump=True)
    assert (plain.begin() == with_jump.begin()).all().item() and (plain.index == with_jump.index).all().item()
    assert with_jump.forced_ids.shape == (3, 16) and with_jump.forced_len.shape == (3,)
    # nothing is forced at the start of a date: jump() and step() agree
    forced, n = with_jump.jump()
    plain.step(None)
    assert n.cpu().tolist() == [0, 0, 0] and (plain.mask == with_jump.mask).all().item() and (plain.state == with_jump.state).all().item()
