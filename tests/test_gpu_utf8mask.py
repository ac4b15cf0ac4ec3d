"""GPU tests (-m gpu): spl_utf8_mask_device -- allowed-token bitmasks from the stream decoder's state words -- through the C ABI into guarded
buffers against the rule of tests/utf8_mask_ref.py, bit for bit: the toy vocabulary with every state in one batch, every id of three
shipped vocabularies in the eight classes, batch sizes and row widths around the kernels' edges, skip_special_tokens, and_into, live, the
table rebuilt after spl_add_special; the closed loop with the batched streaming decode (no sequence ever stalls); the refusals."""
import ctypes

import numpy as np
import pytest

import utf8_mask_ref as ref
import vocabgen

pytestmark = pytest.mark.gpu

MASK_POISON = 0x5A5A5A5A
PATTERN = r"[a-z]+|\s+|[^a-z\s]+"
AND, SKIP = 1, 4

_toy_tok = {}


def _toy(tmp_path_factory):
    """(tokenizer, vocab, specials).  The file holds the empty token too: the loader drops an empty key (it can never match a chunk), so
    to the library its id is a hole -- the reference gets the vocabulary without it."""
    if not _toy_tok:
        from splintr_amd import Tokenizer
        full, specials = ref.toy()
        path = tmp_path_factory.mktemp("utf8mask") / "toy.tiktoken"
        path.write_bytes(vocabgen.tiktoken({b: i for i, b in full.items()}))
        tok = Tokenizer(str(path), PATTERN, {v.decode(): k for k, v in specials.items()})
        vocab, _ = ref.toy(with_empty=False)
        assert tok.vocab_size == max(specials) + 1 and tok._token_bytes(ref.toy_empty_id(), True) is None
        _toy_tok["t"] = (tok, vocab, specials)
    return _toy_tok["t"]


def _call(tok, words, *, skip=False, n_words, and_into=None, want_live=True):
    """One call through the C ABI with poisoned outputs and a spare row behind each -> (mask uint32 [B, n_words], live uint8 [B]); asserts
    that nothing behind the rows was written."""
    import torch
    from splintr_amd import _ffi
    dev = torch.device("cuda", 0)
    B = len(words)
    state = torch.from_numpy(np.asarray(list(words) + [0], dtype=np.uint64).view(np.int64)).to(dev)
    t_mask = torch.full((B + 1, n_words), MASK_POISON, dtype=torch.int32, device=dev)
    if and_into is not None and B:
        t_mask[:B] = torch.from_numpy(np.asarray(and_into, dtype=np.uint32).view(np.int32)).to(dev)
    t_live = torch.full((B + 1,), 0x5A, dtype=torch.uint8, device=dev)
    o = _ffi.SplDecodeOpts(SKIP if skip else 0, 1)
    rc = _ffi.lib().spl_utf8_mask_device(tok.handle, state.data_ptr(), B, ctypes.byref(o), AND if and_into is not None else 0, n_words,
                                         t_mask.data_ptr(), t_live.data_ptr() if want_live else None, torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, _ffi.last_error()
    mask, live = t_mask.cpu().numpy().view(np.uint32), t_live.cpu().numpy()
    assert (mask[B] == MASK_POISON).all() and live[B] == 0x5A, "written behind the rows"
    if not want_live:
        assert (live == 0x5A).all()
    return mask[:B].copy(), live[:B].copy()


_want = {}


def _toy_want(vocab, specials, words, skip, n_words):
    key = (tuple(words), skip, n_words)
    if key not in _want:
        _want[key] = ref.masks(vocab, specials, words, skip, n_words)
    return _want[key]


# ---------------------------------------------------------------------------------------------- the toy vocabulary
@pytest.mark.parametrize("skip", [False, True])
def test_toy_every_state_in_one_batch(skip, tmp_path_factory):
    tok, vocab, specials = _toy(tmp_path_factory)
    words = [w for _, w in ref.toy_states()]
    nw0 = (tok.vocab_size + 31) // 32
    for n_words in (nw0, nw0 + 1, 2 * nw0, (nw0 + 3) & ~3):                      # (the last a multiple of four: the 16-byte lanes)
        want, want_live = _toy_want(vocab, specials, words, skip, n_words)
        got, live = _call(tok, words, skip=skip, n_words=n_words)
        assert (got == want).all() and (live == want_live).all(), n_words
        bits = np.unpackbits(got.view(np.uint8), axis=1, bitorder="little")
        assert (bits[want_live == 1][:, tok.vocab_size:] == 0).all()            # the bits beyond the largest known id


@pytest.mark.parametrize("B", [0, 1, 63, 64, 65, 257])
def test_batch_sizes(B, tmp_path_factory):
    tok, vocab, specials = _toy(tmp_path_factory)
    states = [w for _, w in ref.toy_states()]
    words = [states[(7 * i) % len(states)] for i in range(B)]
    for n_words in ((tok.vocab_size + 31) // 32, ((tok.vocab_size + 31) // 32 + 3) & ~3):
        base, base_live = _toy_want(vocab, specials, states, False, n_words)
        idx = [(7 * i) % len(states) for i in range(B)]
        got, live = _call(tok, words, n_words=n_words)
        assert got.shape == (B, n_words) and (got == base[idx]).all() and (live == base_live[idx]).all()


def test_and_into_and_no_live(tmp_path_factory):
    tok, vocab, specials = _toy(tmp_path_factory)
    words = [w for _, w in ref.toy_states()]
    rng = np.random.default_rng(3)
    for n_words in ((tok.vocab_size + 31) // 32 + 1, ((tok.vocab_size + 31) // 32 + 3) & ~3):
        other = rng.integers(0, 1 << 32, size=(len(words), n_words), dtype=np.uint64).astype(np.uint32)
        want, want_live = _toy_want(vocab, specials, words, True, n_words)
        got, live = _call(tok, words, skip=True, n_words=n_words, and_into=other)
        assert (got == (want & other)).all() and (live == want_live).all()
        got, _ = _call(tok, words, skip=True, n_words=n_words, want_live=False)
        assert (got == want).all()


def test_python_surface(tmp_path_factory):
    import torch
    from splintr_amd import device as dv
    tok, vocab, specials = _toy(tmp_path_factory)
    words = [w for _, w in ref.toy_states()]
    state = torch.from_numpy(np.asarray(words, dtype=np.uint64).view(np.int64)).cuda()
    dv.utf8_mask_reserve(tok)
    mask, live = dv.utf8_mask_device(tok, state)
    want, want_live = _toy_want(vocab, specials, words, False, (tok.vocab_size + 31) // 32)
    assert (mask.cpu().numpy().view(np.uint32) == want).all() and (live.cpu().numpy() == want_live).all()
    out = torch.full((len(words), 16), 0x0F0F0F0F, dtype=torch.int32, device=state.device)
    m2, _ = dv.utf8_mask_device(tok, state, out=out, and_into=True, skip_special_tokens=True)
    want16, _ = _toy_want(vocab, specials, words, True, 16)
    assert m2 is out and (out.cpu().numpy().view(np.uint32) == (want16 & 0x0F0F0F0F)).all()
    for bad, word in ((dict(state=state.to(torch.int32)), "int64"), (dict(state=state.cpu()), "on a GPU"), (dict(state=state, n_words=0), "n_words"),
                      (dict(state=state, out=out[:, :5]), "contiguous int32"), (dict(state=state, and_into=True), "and_into needs out"),
                      (dict(state=state, out=out.cpu()), "device of state"), (dict(state=state.reshape(-1, 1)), "shape")):
        st = bad.pop("state")
        with pytest.raises(ValueError, match=word):
            dv.utf8_mask_device(tok, st, **bad)
    with pytest.raises(ValueError, match="n_words is too small"):
        dv.utf8_mask_device(tok, state, n_words=(tok.vocab_size + 31) // 32 - 1)


# ---------------------------------------------------------------------------------------------- the shipped vocabularies, every id
def _known(tok):
    """[(id, bytes the decode emits)] of the vocabulary proper and of the special map, apart"""
    from splintr_amd import _ffi
    L = _ffi.lib()
    voc, sp = [], []
    p, n = ctypes.c_void_p(), ctypes.c_uint32()
    for i in range(tok.vocab_size):
        kind = L.spl_token_bytes(tok.handle, i, ctypes.byref(p), ctypes.byref(n))
        if kind:
            (sp if kind == 3 else voc).append((i, ctypes.string_at(p, n.value) if n.value else b""))
    return voc, sp


def _class_words():
    return [ref.state_word(p) for p in ref.CLASS_REPS]


def _shipped_want(voc, sp, nw):
    tab_v, tab_s = ref.class_table(voc, nw), ref.class_table(sp, nw)
    any_s = np.zeros(nw * 32, dtype=np.uint8)
    any_s[[i for i, _ in sp]] = 1
    return tab_v, tab_s, np.packbits(any_s, bitorder="little").view(np.uint32)


@pytest.mark.parametrize("name", ["cl100k_base", "o200k_base", "deepseek_v3"])
def test_every_id_of_a_shipped_vocabulary(name):
    from splintr_amd import Tokenizer
    tok = Tokenizer.from_pretrained(name)
    voc, sp = _known(tok)
    assert len(sp) >= 1 and len(voc) > 90000
    nw = (tok.vocab_size + 31) // 32 + 1
    tab_v, tab_s, any_s = _shipped_want(voc, sp, nw)
    got, live = _call(tok, _class_words(), n_words=nw)
    assert (got == (tab_v | tab_s)).all() and (live == 1).all()
    got, _ = _call(tok, _class_words(), skip=True, n_words=nw)
    assert (got == (tab_v | any_s[None, :])).all()
    # thousands of ids are fragments of characters: the start row forbids some, every other row allows some
    pop = np.unpackbits((tab_v | tab_s).view(np.uint8), axis=1, bitorder="little").sum(1)
    assert pop[0] < len(voc) + len(sp) and (pop[1:] >= 1).all() and (pop[1:] < pop[0]).all()


def test_table_is_rebuilt_after_add_special():
    from splintr_amd import Tokenizer, _ffi
    tok = Tokenizer.from_pretrained("cl100k_base")
    nw = (tok.vocab_size + 31) // 32 + 4
    before, _ = _call(tok, _class_words(), n_words=nw)
    new_id = tok.vocab_size + 70                                               # beyond every id so far: a wider table
    lit = "<|café|>".encode()
    assert _ffi.lib().spl_add_special(tok.handle, lit, len(lit), new_id) == 0
    assert new_id >> 5 < nw
    after, _ = _call(tok, _class_words(), n_words=nw)
    want = before.copy()
    want[0, new_id >> 5] |= np.uint32(1 << (new_id & 31))                       # ASCII first: from the start alone
    assert (after == want).all()
    skipped, _ = _call(tok, _class_words(), skip=True, n_words=nw)
    assert all((skipped[c, new_id >> 5] >> (new_id & 31)) & 1 for c in range(8))
    with pytest.raises(AssertionError, match="n_words is too small"):
        _call(tok, _class_words(), n_words=(new_id >> 5))


# ---------------------------------------------------------------------------------------------- the closed loop
def _closed_loop(tok, B=64, steps=200, seed=5):
    import torch
    torch.manual_seed(seed)
    dec = tok.device_streaming_decoder(B, errors="hold")
    dev = dec.state.device
    shifts = torch.arange(32, device=dev, dtype=torch.int32)
    texts, drawn = [""] * B, []
    for _ in range(steps):
        mask, live = dec.allowed_mask()
        bits = ((mask.unsqueeze(-1) >> shifts) & 1).reshape(B, -1).to(torch.float32)
        ids = torch.multinomial(bits, 1).reshape(B)                             # uniform over the row's allowed ids
        drawn.append(ids)
        for b, t in enumerate(dec.add_tokens(ids.to(torch.int32))):
            texts[b] += t or ""
    assert not dec.stalled.any().item() and live.all().item()
    tail = dec.flush()
    ids = torch.stack(drawn, 1).cpu().tolist()
    pend = 0
    for b in range(B):
        raw = b"".join(tok._token_bytes(t, True) for t in ids[b])
        assert texts[b] + (tail[b] or "") == raw.decode("utf-8", "replace"), b
        assert texts[b].encode() == raw[:len(texts[b].encode())] and ref.is_beginning(raw[len(texts[b].encode()):])
        pend += bool(tail[b])
    return pend


def test_closed_loop_toy(tmp_path_factory):
    tok, _, _ = _toy(tmp_path_factory)
    assert _closed_loop(tok) >= 1                                              # the toy vocabulary leaves characters unfinished all the time


def test_closed_loop_cl100k():
    from splintr_amd import Tokenizer
    _closed_loop(Tokenizer.from_pretrained("cl100k_base"))


def test_toy_forbidden_ids_stall_the_decoder(tmp_path_factory):
    """from each representative state: a known id whose bit is 0 stalls the hold-mode decode, one whose bit is 1 does not"""
    import torch
    from splintr_amd import device as dv
    tok, vocab, specials = _toy(tmp_path_factory)
    known = sorted(set(vocab) | set(specials))
    words = [ref.state_word(p) for p in ref.CLASS_REPS]
    nw = (tok.vocab_size + 31) // 32
    mask, _ = _call(tok, words, n_words=nw)
    pairs = [(c, t) for c in range(8) for t in known]
    state = torch.from_numpy(np.asarray([words[c] for c, _ in pairs], dtype=np.uint64).view(np.int64)).cuda()
    ids = torch.tensor([[t] for _, t in pairs], dtype=torch.int32, device=state.device)
    _, _, out = dv.stream_decode_device(tok, ids, None, state, errors="hold", max_bytes=64 * len(pairs))
    stalled = ((out.cpu().numpy().view(np.uint64) >> 26) & 1).astype(bool)
    allowed = np.array([(int(mask[c, t >> 5]) >> (t & 31)) & 1 for c, t in pairs], dtype=bool)
    assert (stalled == ~allowed).all() and stalled.any() and allowed.any()


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals(tmp_path_factory):
    import torch
    from splintr_amd import _ffi
    tok, vocab, specials = _toy(tmp_path_factory)
    L = _ffi.lib()
    dev = torch.device("cuda", 0)
    nw = (tok.vocab_size + 31) // 32
    state = torch.zeros(4, dtype=torch.int64, device=dev)
    mask = torch.zeros((2, nw), dtype=torch.int32, device=dev)
    live = torch.zeros(8, dtype=torch.uint8, device=dev)
    o = _ffi.SplDecodeOpts(0, 1)

    def go(word, *, h=tok.handle, st=state.data_ptr(), n=2, opts=o, flags=0, n_words=nw, m=mask.data_ptr(), lv=live.data_ptr()):
        assert L.spl_utf8_mask_device(h, st, n, ctypes.byref(opts) if opts is not None else None, flags, n_words, m, lv, None) == -1, word
        assert word in _ffi.last_error(), (word, _ffi.last_error())

    go("null handle", h=None)
    go("options are null", opts=None)
    go("d_state is null", st=None)
    go("d_mask is null", m=None)
    go("n_words is too small", n_words=nw - 1)
    go("n_words is above 2^26", n_words=(1 << 26) + 1)
    go("unknown flag", flags=2)
    go("unknown decode flag", opts=_ffi.SplDecodeOpts(8, 1))
    go("n_seqs >= 2^31", n=1 << 31)
    go("d_state is not 8-byte aligned", st=state.data_ptr() + 4)
    go("d_mask is not 4-byte aligned", m=mask.data_ptr() + 2)
    go("three arrays", lv=mask.data_ptr())
    short = _ffi.SplDecodeOpts(0, 1)
    short.struct_size = 4
    go("struct_size", opts=short)
    assert L.spl_utf8_mask_reserve_device(None) == -1 and "null handle" in _ffi.last_error()
    assert L.spl_utf8_mask_device(tok.handle, state.data_ptr(), 2, ctypes.byref(o), 0, nw, mask.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
