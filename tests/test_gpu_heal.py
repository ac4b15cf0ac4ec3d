"""GPU tests (-m gpu): spl_heal_begin_device / spl_heal_step_device -- token healing, allowed-token bitmasks from byte prefixes -- through
the C ABI into guarded buffers against the definition of tests/heal_ref.py: the toy enumerations of tests/heal_cases.py as one batch per
vocabulary, batch sizes and vocabulary sizes around the kernels' edges, the refusals, the shipped vocabularies end to end against a numpy
brute force, and TokenHealer."""
import ctypes
import json
import os

import numpy as np
import pytest

import heal_cases as cases
import heal_ref as ref
import vocabgen

pytestmark = pytest.mark.gpu

WORD_POISON = 0x5A5A5A5A5A5A5A5A
MASK_POISON = 0x5A5A5A5A
AUTO, KEEP_FREE, I64, PAD_LEFT = 1, 2, 4, 8
WG_IDS = 4096                      # the id range of one fill workgroup (HL_WG_IDS, csrc/spl_k_heal.h)
PATTERN = r"[a-z]+|\s+|[^a-z\s]+"

_toks = {}


def _toy(name, tmp_path_factory):
    """(tokenizer, ordinary tokens, vocab, specials) of a toy vocabulary, built as a tiktoken-format file"""
    if name not in _toks:
        from splintr_amd import Tokenizer
        vocab, specials = (cases.TOYS.get(name) or getattr(cases, "vocab_" + name))()
        path = tmp_path_factory.mktemp("heal") / (name + ".tiktoken")
        path.write_bytes(vocabgen.tiktoken({b: i for i, b in vocab.items()}))
        tok = Tokenizer(str(path), PATTERN, {v.decode(): k for k, v in specials.items()})
        _toks[name] = (tok, ref.ordinary(vocab), vocab, specials)
    return _toks[name]


def _call(tok, *, begin, ids, lengths=None, state=None, flags=0, max_back=0, min_keep=0, n_words, in_place=False, mask_init=None, want=True):
    """One call through the C ABI with poisoned outputs and a spare row behind each -> dict of numpy arrays; asserts that nothing behind
    the rows was written."""
    import torch
    from splintr_amd import _ffi
    dev = torch.device("cuda", 0)
    ids = np.ascontiguousarray(ids)
    B, K = ids.shape
    if ids.dtype == np.int64:
        flags |= I64
    t_ids = torch.from_numpy(ids.view(np.int32) if ids.dtype == np.uint32 else ids).to(dev)
    t_len = None if lengths is None else torch.from_numpy(np.ascontiguousarray(lengths, dtype=np.int32)).to(dev)
    t_sin = None
    if not begin:
        rows = np.concatenate([np.asarray(state, dtype=np.uint64).reshape(B, 9), np.full((1, 9), WORD_POISON, dtype=np.uint64)])
        t_sin = torch.from_numpy(rows.view(np.int64)).to(dev)
    t_sout = t_sin if in_place else torch.full((B + 1, 9), WORD_POISON, dtype=torch.int64, device=dev)
    t_mask = torch.full((B + 1, n_words), MASK_POISON, dtype=torch.int32, device=dev)
    if mask_init is not None:
        t_mask[:B] = torch.from_numpy(np.asarray(mask_init, dtype=np.uint32).view(np.int32)).to(dev)
    t_live = torch.full((B + 1,), 0x5A, dtype=torch.uint8, device=dev)
    t_nb = torch.full((B + 1,), MASK_POISON, dtype=torch.int32, device=dev)
    t_n = torch.full((3,), -7, dtype=torch.int32, device=dev)
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    si = _ffi.SplHealIn(B, K, ptr(t_ids), ptr(t_len), ptr(t_sin))
    o = _ffi.SplHealOpts(flags, n_words, max_back, min_keep)
    so = _ffi.SplHealOut(t_sout.data_ptr(), t_mask.data_ptr(), t_live.data_ptr() if want else None, t_n.data_ptr() if want else None,
                         t_nb.data_ptr() if begin else None)
    L = _ffi.lib()
    fn = L.spl_heal_begin_device if begin else L.spl_heal_step_device
    rc = fn(tok.handle, ctypes.byref(si), ctypes.byref(o), ctypes.byref(so), torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, _ffi.last_error()
    st = t_sout.cpu().numpy().view(np.uint64)
    mask = t_mask.cpu().numpy().view(np.uint32)
    live, nb, n = t_live.cpu().numpy(), t_nb.cpu().numpy(), t_n.cpu().numpy()
    assert (st[B] == WORD_POISON).all() and (mask[B] == MASK_POISON).all() and live[B] == 0x5A and nb[B] == MASK_POISON and n[2] == -7, \
        "written behind the rows"
    if not begin:
        assert (nb == MASK_POISON).all()
    if not want:
        assert (live == 0x5A).all() and (n == -7).all()
    return dict(state=st[:B].copy(), mask=mask[:B].copy(), live=live[:B].copy(), n_back=nb[:B].copy(), n=n[:2].copy())


def _min_words(vocab):
    return (max(vocab) + 32) // 32


_ref_rows = {}


def _want_mask(name, toks, P, n_words):
    key = (name, P, n_words)
    if key not in _ref_rows:
        _ref_rows[key] = ref.mask_words(toks, P, n_words)
    return _ref_rows[key]


# ---------------------------------------------------------------------------------------------- the toy enumerations
@pytest.mark.parametrize("name", sorted(cases.TOYS))
def test_toy_masks_of_every_prefix_in_one_batch(name, tmp_path_factory):
    tok, toks, vocab, specials = _toy(name, tmp_path_factory)
    ps = [b""] + cases.prefixes(name)
    for n_words in (_min_words(vocab), _min_words(vocab) + 3):                # the surplus: ones when free, zeros when constrained
        r = _call(tok, begin=False, ids=np.zeros((len(ps), 0), dtype=np.int32), state=cases.state_rows(ps), n_words=n_words)
        for p, row in zip(ps, r["mask"]):
            assert row.tolist() == _want_mask(name, toks, p, n_words).tolist(), p
        assert r["live"].tolist() == [int(len(p) > 0) for p in ps] and r["n"].tolist() == [len(ps) - 1, 0]
        assert (r["state"] == cases.state_rows(ps)).all()


@pytest.mark.parametrize("name", sorted(cases.TOYS))
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_toy_one_step_with_every_id_in_one_batch(name, dtype, tmp_path_factory):
    tok, toks, vocab, specials = _toy(name, tmp_path_factory)
    pool = cases.probe_ids(vocab, specials)
    ps = [b""] + cases.prefixes(name)[:120] + (cases.EDGE_PREFIXES if name == "edges" else [])
    pairs = [(p, t) for p in ps for t in pool]
    ids = np.array([[t] for _, t in pairs], dtype=np.uint32)
    ids = ids.view(np.int32) if dtype == np.int32 else ids.astype(np.int64)
    nw = _min_words(vocab)
    r = _call(tok, begin=False, ids=ids, state=cases.state_rows([p for p, _ in pairs]), n_words=nw, in_place=(dtype == np.int64))
    broke = 0
    for (p, t), row, m in zip(pairs, r["state"], r["mask"]):
        want = ref.step(toks, (p, False, False), [t])
        assert row.tolist() == ref.state_row(want).tolist(), (p, t)
        assert m.tolist() == _want_mask(name, toks, want[0], nw).tolist(), (p, t)
        broke += want[1]
    assert r["n"].tolist() == [int(r["live"].sum()), broke]


@pytest.mark.parametrize("name", sorted(cases.TOYS))
def test_toy_steps_at_every_cut(name, tmp_path_factory):
    tok, toks, vocab, specials = _toy(name, tmp_path_factory)
    sc = cases.step_cases(name)
    ps, seqs = [p for p, _ in sc], [ids for _, ids in sc]
    K, nw = len(seqs[0]), _min_words(vocab)
    want = np.stack([ref.state_row(ref.step(toks, (p, False, False), ids)) for p, ids in sc])
    feed = lambda st, part, dt, **kw: _call(tok, begin=False, ids=cases.rows_of(part, max(len(part[0]), 1), dt)[0][:, :len(part[0])], state=st,
                                            n_words=nw, **kw)
    whole = feed(cases.state_rows(ps), seqs, np.int32)
    assert (whole["state"] == want).all()
    for m, w in zip(whole["mask"], want):
        assert m.tolist() == _want_mask(name, toks, ref.row_state(w)[0], nw).tolist()
    st = cases.state_rows(ps)
    for k in range(K):
        st = feed(st, [s[k:k + 1] for s in seqs], np.int64, in_place=True)["state"]
    assert (st == want).all()
    for cut in range(1, K):
        a = feed(cases.state_rows(ps), [s[:cut] for s in seqs], np.int32)["state"]
        b = feed(a, [s[cut:] for s in seqs], np.int64)
        assert (b["state"] == want).all() and (b["mask"] == whole["mask"]).all()
    rows, _ = cases.rows_of(seqs, K, np.int32)
    lens = np.array([i % (K + 2) - 1 for i in range(len(seqs))], dtype=np.int32)
    r = _call(tok, begin=False, ids=rows, lengths=lens, state=cases.state_rows(ps), n_words=nw, want=False)
    for (p, ids), n, row in zip(sc, lens, r["state"]):
        assert row.tolist() == ref.state_row(ref.step(toks, (p, False, False), ids[:max(int(n), 0)])).tolist()


@pytest.mark.parametrize("name", sorted(cases.TOYS))
@pytest.mark.parametrize("auto", [False, True])
def test_toy_begin_over_every_limit(name, auto, tmp_path_factory):
    tok, toks, vocab, specials = _toy(name, tmp_path_factory)
    prompts, nw = cases.prompts(name), _min_words(vocab)
    for max_back in range(9):
        side, dtype, min_keep = [("right", np.int32, 0), ("left", np.int64, 1), ("right", np.int64, 2)][max_back % 3]
        rows, lens = cases.rows_of(prompts, 8, dtype, side)
        flags = (AUTO if auto else 0) | (PAD_LEFT if side == "left" else 0)
        r = _call(tok, begin=True, ids=rows, lengths=lens, flags=flags, max_back=max_back, min_keep=min_keep, n_words=nw)
        for pr, nb, row, m in zip(prompts, r["n_back"], r["state"], r["mask"]):
            want = ref.begin(toks, pr, max_back=max_back, min_keep=min_keep, auto=auto)
            assert (int(nb), ref.row_state(row)) == (want[0], (want[1], False, False)), (pr, max_back, min_keep, side)
            assert m.tolist() == _want_mask(name, toks, want[1], nw).tolist()
        assert r["n"].tolist() == [int(r["live"].sum()), 0]


def test_long_prefixes_and_long_covering_tokens(tmp_path_factory):
    tok, toks, vocab, specials = _toy("long", tmp_path_factory)
    nw = _min_words(vocab)
    ps = [b"a", b"a" * 63, b"a" * 64, b"a" * 63 + b"b", b"a" * 62 + b"b", b"b", b"a" * 33]
    r = _call(tok, begin=False, ids=np.zeros((len(ps), 0), dtype=np.int32), state=cases.state_rows(ps), n_words=nw)
    for p, row in zip(ps, r["mask"]):
        assert row.tolist() == ref.mask_words(toks, p, nw).tolist(), p
    ids = np.array([[65, 0], [62, 64], [62, 67]], dtype=np.int32)                 # a^128 | a^63 a^65 | a^63 b
    r = _call(tok, begin=False, ids=ids, state=cases.state_rows([b"a" * 64] * 3), n_words=nw)
    assert [ref.row_state(x) for x in r["state"]] == [(b"", False, True), (b"", False, True), (b"", True, False)]
    prompts = [[31, 31, 0], [31, 31], [63, 0], [64, 0], [65]]
    rows, lens = cases.rows_of(prompts, 3, np.int32)
    r = _call(tok, begin=True, ids=rows, lengths=lens, max_back=8, n_words=nw)
    assert r["n_back"].tolist() == [2, 2, 1, 1, 0]
    for pr, row in zip(prompts, r["state"]):
        assert ref.row_state(row)[0] == ref.begin(toks, pr, max_back=8)[1]


def test_keep_free_leaves_free_rows_alone(tmp_path_factory):
    tok, toks, vocab, specials = _toy("gaps", tmp_path_factory)
    nw = _min_words(vocab) + 1
    ps = [b"", b"ab", b"", b"c", b"zz", b""]
    init = np.arange(len(ps) * nw, dtype=np.uint32).reshape(len(ps), nw) + 77
    ids = np.array([[0], [3], [0], [0], [0], [0]], dtype=np.int32)
    r = _call(tok, begin=False, ids=ids, state=cases.state_rows(ps), flags=KEEP_FREE, n_words=nw, mask_init=init)
    assert r["live"].tolist() == [0] * len(ps) and (r["mask"] == init).all() and r["n"].tolist() == [0, 2]
    r = _call(tok, begin=False, ids=ids[:, :0], state=cases.state_rows(ps), flags=KEEP_FREE, n_words=nw, mask_init=init)
    for p, row, keep in zip(ps, r["mask"], init):
        assert row.tolist() == (ref.mask_words(toks, p, nw).tolist() if p else keep.tolist())


# ---------------------------------------------------------------------------------------------- batch sizes, vocabulary sizes
@pytest.mark.parametrize("B", [0, 1, 15, 16, 17, 63, 64, 65, 1025])
def test_batch_sizes(B, tmp_path_factory):
    tok, toks, vocab, specials = _toy("gaps", tmp_path_factory)
    nw = _min_words(vocab)
    pool = [b""] + cases.prefixes("gaps")[:40]
    ps = [pool[(7 * i) % len(pool)] for i in range(B)]
    ids = np.array([[(3 * i) % 36] for i in range(B)], dtype=np.int32).reshape(B, 1)
    r = _call(tok, begin=False, ids=ids, state=cases.state_rows(ps), n_words=nw)
    live = 0
    for p, t, row, m in zip(ps, ids[:, 0], r["state"], r["mask"]):
        want = ref.step(toks, (p, False, False), [int(t)])
        assert row.tolist() == ref.state_row(want).tolist() and m.tolist() == _want_mask("gaps", toks, want[0], nw).tolist()
        live += bool(want[0])
    assert int(r["n"][0]) == live == int(r["live"].sum())


def _sized_vocab(n):
    """n tokens, ids 0 .. n - 1: the strings of 1 .. 3 lower-case letters in id order by a fixed shuffle"""
    import itertools
    import random
    al = b"abcdefghijklmnopqrstuvwxyz"
    toks = [bytes(t) for k in (1, 2, 3) for t in itertools.product(al, repeat=k)][:n]
    random.Random(5).shuffle(toks)
    return dict(enumerate(toks))


@pytest.mark.parametrize("past", [31, 32, 33, 63, 64, 65])
def test_vocabulary_sizes_around_the_fill_workgroup(past, tmp_path_factory):
    from splintr_amd import Tokenizer
    vocab = _sized_vocab(WG_IDS + past)
    path = tmp_path_factory.mktemp("heal") / ("sized%d.tiktoken" % past)
    path.write_bytes(vocabgen.tiktoken({b: i for i, b in vocab.items()}))
    tok = Tokenizer(str(path), PATTERN, {})
    toks = ref.ordinary(vocab)
    ps = [b"", b"a", b"ab", b"abc", b"zz", b"b", b"abcd", b"q"]
    for nw in (_min_words(vocab), _min_words(vocab) + 3):
        r = _call(tok, begin=False, ids=np.zeros((len(ps), 0), dtype=np.int32), state=cases.state_rows(ps), n_words=nw)
        for p, row in zip(ps, r["mask"]):
            assert (row == ref.mask_words(toks, p, nw)).all(), p


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals(tmp_path_factory):
    import torch
    from splintr_amd import _ffi, device as dv
    tok, toks, vocab, specials = _toy("gaps", tmp_path_factory)
    L = _ffi.lib()
    dev = torch.device("cuda", 0)
    nw = _min_words(vocab)
    ids = torch.zeros((2, 2), dtype=torch.int32, device=dev)
    lens = torch.ones(2, dtype=torch.int32, device=dev)
    st = torch.zeros((2, 9), dtype=torch.int64, device=dev)
    st2 = torch.zeros((2, 9), dtype=torch.int64, device=dev)
    mask = torch.zeros((2, nw), dtype=torch.int32, device=dev)
    nb = torch.zeros(2, dtype=torch.int32, device=dev)
    n = torch.zeros(2, dtype=torch.int32, device=dev)

    def go(begin, si, o, so, word):
        fn = L.spl_heal_begin_device if begin else L.spl_heal_step_device
        assert fn(tok.handle, ctypes.byref(si), ctypes.byref(o), ctypes.byref(so), None) == -1, word
        assert word in _ffi.last_error(), (word, _ffi.last_error())

    I = lambda **kw: _ffi.SplHealIn(2, 2, kw.get("ids", ids.data_ptr()), kw.get("lens", lens.data_ptr()), kw.get("state", st.data_ptr()))
    O = lambda **kw: _ffi.SplHealOut(kw.get("state", st2.data_ptr()), kw.get("mask", mask.data_ptr()), None, kw.get("n", n.data_ptr()),
                                     kw.get("nb", nb.data_ptr()))
    go(False, I(), _ffi.SplHealOpts(0, nw - 1), O(), "n_words is too small")
    go(True, I(), _ffi.SplHealOpts(0, nw, 9), O(), "max_back")
    go(False, I(state=None), _ffi.SplHealOpts(0, nw), O(), "d_state_in is null")
    go(False, I(), _ffi.SplHealOpts(0, nw), O(state=None), "d_state_out is null")
    go(False, I(), _ffi.SplHealOpts(0, nw), O(mask=None), "d_mask is null")
    go(True, I(), _ffi.SplHealOpts(0, nw), O(nb=None), "d_n_back is null")
    go(True, I(ids=None), _ffi.SplHealOpts(0, nw), O(), "d_ids is null")
    go(True, I(lens=None), _ffi.SplHealOpts(PAD_LEFT, nw), O(), "needs d_len")
    go(False, I(), _ffi.SplHealOpts(AUTO, nw), O(), "unknown flag bit")
    go(False, I(), _ffi.SplHealOpts(PAD_LEFT, nw), O(), "unknown flag bit")
    go(True, I(), _ffi.SplHealOpts(64, nw), O(), "unknown flag bit")
    go(False, I(), _ffi.SplHealOpts(0, nw), O(mask=ids.data_ptr()), "coincides with an input")
    go(False, I(), _ffi.SplHealOpts(0, nw), O(n=lens.data_ptr()), "coincides with an input")
    go(False, I(), _ffi.SplHealOpts(0, nw), O(mask=st.data_ptr()), "coincides with an input")
    go(True, I(), _ffi.SplHealOpts(0, nw), O(nb=n.data_ptr()), "coincides with d_n")
    go(False, I(ids=ids.data_ptr() + 4), _ffi.SplHealOpts(I64, nw), O(), "not aligned")
    o = _ffi.SplHealOpts(0, nw)
    o.struct_size = 8
    go(False, I(), o, O(), "struct_size")
    # state out with state in is the one overlap allowed
    assert L.spl_heal_step_device(tok.handle, ctypes.byref(I()), ctypes.byref(_ffi.SplHealOpts(0, nw)), ctypes.byref(O(state=st.data_ptr())), None) == 0
    torch.cuda.synchronize()
    # the Python layer: dtypes, shapes, sizes
    with pytest.raises(ValueError, match="int32 or int64"):
        dv.heal_step_device(tok, ids.to(torch.int16), None, st)
    with pytest.raises(ValueError, match="max_back"):
        dv.heal_begin_device(tok, ids, lens, max_back=9)
    with pytest.raises(ValueError, match="n_words is too small"):
        dv.heal_begin_device(tok, ids, lens, n_words=nw - 1)
    with pytest.raises(ValueError, match="needs lengths"):
        dv.heal_begin_device(tok, ids, None, padding_side="left")
    with pytest.raises(ValueError, match="keep_free needs"):
        dv.heal_step_device(tok, ids, None, st, keep_free=True)
    with pytest.raises(ValueError, match="at most 64"):
        dv.heal_state_from_prefixes([b"x" * 65])


# ---------------------------------------------------------------------------------------------- the shipped vocabularies, end to end
def _matrix(tok):
    """(ordinary tokens, ids [n], bytes [n, 64] zero padded and cut, lengths [n]) of a shipped vocabulary"""
    toks = []
    for i in range(tok.vocab_size):
        p, n = ctypes.c_void_p(), ctypes.c_uint32()
        from splintr_amd import _ffi
        if _ffi.lib().spl_token_bytes(tok.handle, i, ctypes.byref(p), ctypes.byref(n)) in (1, 2) and n.value:
            toks.append((i, ctypes.string_at(p, n.value)))
    M = np.zeros((len(toks), 64), dtype=np.uint8)
    for r, (_, b) in enumerate(toks):
        M[r, :min(len(b), 64)] = np.frombuffer(b[:64], dtype=np.uint8)
    return toks, np.array([i for i, _ in toks], dtype=np.int64), M, np.array([len(b) for _, b in toks], dtype=np.int64)


def _np_allowed(ids, M, lens, P):
    """brute force: the covering and the partial ids of P"""
    p = np.frombuffer(P, dtype=np.uint8)
    eq = M[:, :len(P)] == p
    lead = np.where(eq.all(1), len(P), (~eq).argmax(1))                         # bytes shared at the front
    return ids[((lead == len(P)) & (lens >= len(P))) | ((lens < len(P)) & (lead >= lens))]


def _np_begin(toks_by_id, ids, M, lens, prompt, max_back, auto):
    P, j = b"", 1
    while j <= max_back and len(prompt) - j >= 0:
        b = toks_by_id.get(prompt[-j])
        if b is None or len(b) + len(P) > 64:
            break
        cand = b + P
        if auto:
            c = np.frombuffer(cand, dtype=np.uint8)
            if not ((lens > len(cand)) & (M[:, :len(cand)] == c).all(1)).any():
                break
        P, j = cand, j + 1
    return j - 1, P


@pytest.mark.parametrize("name", ["cl100k_base", "o200k_base", "deepseek_v3"])
def test_shipped_vocabulary_end_to_end(name):
    from splintr_amd import Tokenizer, corpus
    from conftest import ROOT
    tok = Tokenizer.from_pretrained(name)
    toks, ids, M, lens = _matrix(tok)
    by_id = dict(toks)
    with open(os.path.join(ROOT, "tests", "golden", "corpus_fixtures.json")) as f:
        ent = json.load(f)["c2_cl100k"]
    texts = getattr(corpus, ent["generator"])(ent["n"], **ent.get("kwargs", {}))
    prompts, fulls = [], []
    for k, t in enumerate(texts):                                              # cut inside a word: a letter on both sides
        cuts = [c for c in range(8, min(len(t), 200)) if t[c - 1].isascii() and t[c - 1].isalpha() and t[c].isascii() and t[c].isalpha()]
        if cuts:
            c = cuts[(13 * k) % len(cuts)]
            prompts.append(t[:c]); fulls.append(t[:c + 48])
        if len(prompts) == 256:
            break
    assert len(prompts) == 256
    enc, full = tok.encode_batch(prompts), tok.encode_batch(fulls)
    B, K, nw = 256, max(len(e) for e in enc), (tok.vocab_size + 31) // 32 + 3
    rows, ln = cases.rows_of(enc, K, np.int64)
    r = _call(tok, begin=True, ids=rows, lengths=ln, flags=AUTO, max_back=3, n_words=nw)
    states, taken = [], 0
    for b in range(B):
        nb, P = _np_begin(by_id, ids, M, lens, enc[b], 3, True)
        if b < 12:
            assert (nb, P) == ref.begin(toks, enc[b], max_back=3, auto=True)
        assert int(r["n_back"][b]) == nb and ref.row_state(r["state"][b]) == (P, False, False), (b, prompts[b][-20:])
        states.append((P, False, False)); taken += nb
    assert taken >= B // 2                                                      # prompts cut inside a word are rolled back
    st, mask = r["state"], r["mask"]
    kept = [e[:len(e) - int(k)] for e, k in zip(enc, r["n_back"])]
    pos = [len(k) if f[:len(k)] == k else None for k, f in zip(kept, full)]     # where the canonical encoding goes on, if the kept ids begin it
    for step in range(64):
        live = [b for b in range(B) if states[b][0]]
        if not live:
            break
        feed = np.zeros((B, 1), dtype=np.int64)
        ln = np.zeros(B, dtype=np.int32)
        for b in live:
            want = np.zeros(nw * 32, dtype=bool)
            want[_np_allowed(ids, M, lens, states[b][0])] = True
            got = np.unpackbits(mask[b].view(np.uint8), bitorder="little").astype(bool)
            assert (got == want).all(), (name, b, states[b][0])
            t = full[b][pos[b]] if pos[b] is not None and pos[b] < len(full[b]) and want[full[b][pos[b]]] else None
            if t is None:
                pos[b] = None
                t = int(want.argmax()) if want.any() else 0
            else:
                pos[b] += 1
            feed[b, 0], ln[b] = t, 1
            states[b] = ref.step(toks, states[b], [t])
        r = _call(tok, begin=False, ids=feed, lengths=ln, state=st, n_words=nw, in_place=True)
        st, mask = r["state"], r["mask"]
        for b in range(B):
            assert ref.row_state(st[b]) == states[b], (name, step, b)
        assert int(r["n"][0]) == sum(bool(s[0]) for s in states)
    assert not any(s[0] for s in states), "a sequence is still constrained after 64 steps"
    assert (mask.view(np.int32) == -1).all()
    assert sum(s[2] for s in states) >= B // 2


def test_token_healer_end_to_end():
    import torch
    from splintr_amd import Tokenizer
    tok = Tokenizer.from_pretrained("cl100k_base")
    texts = ["The link is http:", "def foo(", "Hello wor", "", "An answer with a trailing space ", "x = np.arr"]
    kept, healer = tok.heal(texts, max_back=2)
    enc = tok.encode_batch(texts)
    n_back = [len(e) - len(k) for e, k in zip(enc, kept)]
    assert all(k == e[:len(k)] for e, k in zip(enc, kept)) and n_back[3] == 0 and sum(n_back) >= 3
    live = healer.live.cpu().numpy().astype(bool)
    assert live.tolist() == [n > 0 for n in n_back] and int(healer.n.cpu()[0]) == int(live.sum())
    pend = healer.pending.cpu().tolist()
    for e, n, p in zip(enc, n_back, pend):
        assert p == len(b"".join(tok._token_bytes(t, True) for t in e[len(e) - n:]))
    V = tok.vocab_size + 5
    torch.manual_seed(3)
    logits = torch.randn((len(texts), V), device=healer.mask.device)
    before = logits.clone()
    healer.apply(logits)
    mask = healer.mask.cpu().numpy().view(np.uint32)
    pick = logits.argmax(1).cpu().tolist()
    for b, t in enumerate(pick):
        if live[b]:
            assert t < 32 * healer.n_words and (int(mask[b, t >> 5]) >> (t & 31)) & 1, (b, t)
            p = b"".join(tok._token_bytes(x, True) for x in enc[b][len(enc[b]) - n_back[b]:])
            tb = tok._token_bytes(t, True)
            assert tb.startswith(p) or (p.startswith(tb) and len(tb) < len(p))
        else:
            assert torch.equal(logits[b], before[b])
    # the sampler's picks go back in; a covering pick heals its sequence
    out = healer.step(torch.tensor(pick, dtype=torch.int64, device=healer.mask.device))
    assert out is healer.mask and not healer.broken.any().item()
    for _ in range(70):
        if not healer.live.any().item():
            break
        row = healer.mask.cpu().numpy().view(np.uint32)
        nxt = [int(np.unpackbits(row[b].view(np.uint8), bitorder="little").argmax()) for b in range(len(texts))]
        healer.step(torch.tensor(nxt, dtype=torch.int32, device=healer.mask.device), healer.live.to(torch.int32))
    assert not healer.live.any().item() and (healer.mask == -1).all().item()
    assert healer.healed.cpu().tolist() == [n > 0 for n in n_back]
    # "the answer must begin with this text": prefixes written into the state rows, the first masks from a step without ids
    from splintr_amd import device as dv
    healer.reset()
    healer.state.copy_(dv.heal_state_from_prefixes(["Sure", "", "{\"", "No", "", ""], healer.mask.device))
    healer.step(None)
    row = healer.mask.cpu().numpy().view(np.uint32)
    sure = tok.encode("Sure")
    assert len(sure) == 1 and (int(row[0, sure[0] >> 5]) >> (sure[0] & 31)) & 1 and (row[1] == 0xFFFFFFFF).all()
    assert healer.live.cpu().tolist() == [1, 0, 1, 1, 0, 0]
