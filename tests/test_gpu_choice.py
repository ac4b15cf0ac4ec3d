"""GPU tests (-m gpu): spl_choice_step_device -- guided choice, allowed-token bitmasks for one-of-N answers -- through the C ABI into guarded
buffers against the definition of tests/choice_ref.py: the checks of tests/choice_cases.py over the toy vocabularies with the row built in
pieces of 4 words and in one piece, batch sizes and vocabulary sizes around the kernel's edges, a mask base off its 16-byte alignment, the
refusals, the shipped vocabularies end to end against a numpy brute force with a uniform sampler, and ChoiceGuide beside the streaming
decode and its UTF-8 mask."""
import ctypes
import random

import numpy as np
import pytest

import choice_cases as cases
import choice_ref as ref
import vocabgen

pytestmark = pytest.mark.gpu

WORD_POISON = 0x5A5A5A5A5A5A5A5A
MASK_POISON = 0x5A5A5A5A
PATTERN = r"[a-z]+|\s+|[^a-z\s]+"
PIECES = [4, 8192]

_toks = {}


def _tok_of(name, vocab, specials, tmp_path_factory):
    if name not in _toks:
        from splintr_amd import Tokenizer
        path = tmp_path_factory.mktemp("choice") / (name + ".tiktoken")
        path.write_bytes(vocabgen.tiktoken({b: i for i, b in vocab.items()}))
        _toks[name] = Tokenizer(str(path), PATTERN, {v.decode(): k for k, v in specials.items()})
    return _toks[name]


def _toy(name, tmp_path_factory):
    vocab, specials = cases.TOYS[name]()
    return _tok_of(name, vocab, specials, tmp_path_factory)


def _set_piece(tok, piece):
    from splintr_amd import _ffi
    assert _ffi.lib().spl_set_option(tok.handle, b"choice_piece_words", piece) == 0, _ffi.last_error()


def _call(tok, table, *, ids, state, lengths=None, flags=0, end_ids=(), n_words, in_place=False, mask_init=None, want_live=True, off16=0):
    """One call through the C ABI with poisoned outputs and a spare row behind each -> dict of numpy arrays; asserts that nothing behind the
    rows was written and that KEEP_FREE left the rows of sequences that are not constrained alone.  off16: words the mask base lies behind
    a 16-byte boundary."""
    import torch
    from splintr_amd import _ffi
    dev = torch.device("cuda", 0)
    ids = np.ascontiguousarray(ids)
    B, K = ids.shape
    if ids.dtype == np.int64:
        flags |= ref.I64
    t_ids = torch.from_numpy(ids.view(np.int32) if ids.dtype == np.uint32 else ids).to(dev)
    t_len = None if lengths is None else torch.from_numpy(np.ascontiguousarray(lengths, dtype=np.int32)).to(dev)
    rows = np.concatenate([np.asarray(state, dtype=np.uint64).reshape(B, 2), np.full((1, 2), WORD_POISON, dtype=np.uint64)])
    t_sin = torch.from_numpy(rows.view(np.int64)).to(dev)
    t_sout = t_sin if in_place else torch.full((B + 1, 2), WORD_POISON, dtype=torch.int64, device=dev)
    flat = torch.full(((B + 1) * n_words + 4,), MASK_POISON, dtype=torch.int32, device=dev)
    t_mask = flat[off16:off16 + (B + 1) * n_words].view(B + 1, n_words)
    assert t_mask.data_ptr() % 16 == 4 * off16
    init = None
    if mask_init is not None:
        init = np.asarray(mask_init, dtype=np.uint32)
        t_mask[:B] = torch.from_numpy(init.view(np.int32)).to(dev)
    t_live = torch.full((B + 1,), 0x5A, dtype=torch.uint8, device=dev)
    t_tab = torch.from_numpy(np.ascontiguousarray(table, dtype=np.uint8)).to(dev)
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    si = _ffi.SplChoiceIn(B, K, ptr(t_ids), ptr(t_len), t_sin.data_ptr(), t_tab.data_ptr())
    o = _ffi.SplChoiceOpts(flags, n_words, end_ids)
    so = _ffi.SplChoiceOut(t_sout.data_ptr(), t_mask.data_ptr(), t_live.data_ptr() if want_live else None)
    rc = _ffi.lib().spl_choice_step_device(tok.handle, ctypes.byref(si), ctypes.byref(o), ctypes.byref(so), torch.cuda.current_stream(dev).cuda_stream)
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
    return lambda table, **kw: _call(tok, table, **dict(fixed, **kw))


# ---------------------------------------------------------------------------------------------- the toy enumerations
@pytest.mark.parametrize("name", sorted(cases.TOYS))
@pytest.mark.parametrize("piece", PIECES)
def test_toy_one_slot_strings_and_every_probe_id(name, piece, tmp_path_factory):
    tok = _toy(name, tmp_path_factory)
    _set_piece(tok, piece)
    try:
        for then_free in (False, True):
            cases.check_one_slot_strings(_runner(tok), name, then_free, extra_words=3 if then_free else 0)
            cases.check_every_probe_id_from_every_state(_runner(tok), name, then_free)
    finally:
        _set_piece(tok, 8192)


@pytest.mark.parametrize("name", sorted(cases.TOYS))
@pytest.mark.parametrize("piece", PIECES)
def test_toy_tables_and_walks(name, piece, tmp_path_factory):
    tok = _toy(name, tmp_path_factory)
    _set_piece(tok, piece)
    try:
        cases.check_tables_and_walks(_runner(tok), name, then_free=(piece == 4), steps=8)
    finally:
        _set_piece(tok, 8192)


@pytest.mark.parametrize("piece", PIECES)
def test_long_edge_end_flags_layout_and_load(piece, tmp_path_factory):
    toks = {n: _toy(n, tmp_path_factory) for n in cases.TOYS}
    for t in toks.values():
        _set_piece(t, piece)
    try:
        cases.check_long_and_edge_choices(lambda name: _runner(toks[name]))
        run = _runner(toks["gaps"])
        cases.check_end_ids_and_flags(run)
        cases.check_layout(run)
        cases.check_load_sanitation(run)
        # a mask whose base is 4 bytes behind a 16-byte boundary: word stores, whatever the row width; no live array
        cases.check_layout(_runner(toks["gaps"], off16=1))
        cases.check_load_sanitation(_runner(toks["gaps"], off16=3))
        vocab, _, _ = cases.toy("gaps")
        r = _call(toks["gaps"], ref.table([b"ab"]), ids=cases.NO_IDS(2), state=cases.rows([ref.begin([b"ab"]), ref.FREE]), end_ids=(4,),
                  n_words=cases.min_words(vocab), want_live=False)
        assert r["state"].tolist() == [[1, 0], [0, 0]] and r["mask"].tolist() == [[0b101, 0], [0xFFFFFFFF] * 2]
    finally:
        for t in toks.values():
            _set_piece(t, 8192)


# ---------------------------------------------------------------------------------------------- batch sizes, vocabulary sizes
@pytest.mark.parametrize("B", [0, 1, 63, 64, 65, 1025])
def test_batch_sizes(B, tmp_path_factory):
    tok = _toy("gaps", tmp_path_factory)
    vocab, specials, toks = cases.toy("gaps")
    nw = cases.min_words(vocab)
    choices = cases.random_table("gaps", 12, 21)
    rng = random.Random(B)
    start = [ref.begin(choices, s) for s in cases.selections(choices, rng, max(B, 4))[:B]]
    ids = [[rng.choice(sorted(vocab))] for _ in range(B)]
    cases.expect(_runner(tok), toks, choices, cases.rows(start), start, np.array(ids, dtype=np.int32).reshape(B, 1), nw, (4, 63))


def _sized_vocab(n):
    """n tokens, ids 0 .. n - 1: the strings of 1 .. 3 lower-case letters in id order by a fixed shuffle"""
    import itertools
    al = b"abcdefghijklmnopqrstuvwxyz"
    toks = [bytes(t) for k in (1, 2, 3) for t in itertools.product(al, repeat=k)][:n]
    random.Random(5).shuffle(toks)
    return dict(enumerate(toks))


@pytest.mark.parametrize("n", [4095, 4096, 4097, 4096 + 97])
def test_vocabulary_sizes_around_a_16_byte_store(n, tmp_path_factory):
    """4 095 and 4 096 ids: 128 words, the row ends at a 16-byte store; 4 097: 129 words, word stores; 4 193: 132 words.  Every width also
    with three words more, in pieces of 64 words and whole, and with the mask base off its alignment."""
    vocab = _sized_vocab(n)
    tok = _tok_of("sized%d" % n, vocab, {}, tmp_path_factory)
    toks = ref.ordinary(vocab)
    choices = [b"abc", b"abd", b"zz", b"q", b"abcabc", b"zzzzzz", vocab[n - 1], vocab[n - 1] + vocab[0]]
    start = [ref.begin(choices, s) for s in (None, [0], [1, 2], [3], [4, 5], [6], [7], [])]
    base = cases.min_words(vocab)
    try:
        for piece in (64, 8192):
            _set_piece(tok, piece)
            for nw, off16 in ((base, 0), (base + 3, 0), (base, 1), (base + 4, 2)):
                end = (32 * nw - 1,)                                              # (at 4 096 ids and 128 words an ordinary id)
                r, states = cases.expect(_runner(tok, off16=off16), toks, choices, cases.rows(start), start, cases.NO_IDS(len(start)), nw, end)
                ids = [[sorted(ref.allowed(toks, choices, st, end))[-1] if st[0] else 0] for st in states]
                cases.expect(_runner(tok, off16=off16), toks, choices, r["state"], states, ids, nw, end, in_place=True)
    finally:
        _set_piece(tok, 8192)


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals(tmp_path_factory):
    import torch
    from splintr_amd import _ffi, device as dv
    tok = _toy("gaps", tmp_path_factory)
    vocab, specials, _ = cases.toy("gaps")
    L = _ffi.lib()
    dev = torch.device("cuda", 0)
    nw = cases.min_words(vocab)
    ids = torch.zeros((2, 2), dtype=torch.int32, device=dev)
    lens = torch.ones(2, dtype=torch.int32, device=dev)
    st = torch.zeros((2, 2), dtype=torch.int64, device=dev)
    st2 = torch.zeros((2, 2), dtype=torch.int64, device=dev)
    mask = torch.zeros((2, nw), dtype=torch.int32, device=dev)
    live = torch.zeros(16, dtype=torch.uint8, device=dev)
    tab = dv.choice_table(["ab", "c"], dev)

    def go(si, o, so, word):
        assert L.spl_choice_step_device(tok.handle, ctypes.byref(si) if si else None, ctypes.byref(o) if o else None, ctypes.byref(so) if so else None,
                                        None) == -1, word
        assert word in _ffi.last_error(), (word, _ffi.last_error())

    I = lambda **kw: _ffi.SplChoiceIn(2, 2, kw.get("ids", ids.data_ptr()), kw.get("lens", lens.data_ptr()), kw.get("state", st.data_ptr()),
                                      kw.get("table", tab.data_ptr()))
    P = lambda flags=0, n_words=nw, end=(4,): _ffi.SplChoiceOpts(flags, n_words, end)
    O = lambda **kw: _ffi.SplChoiceOut(kw.get("state", st2.data_ptr()), kw.get("mask", mask.data_ptr()), kw.get("live", live.data_ptr()))
    go(None, P(), O(), "the input struct is null")
    go(I(), None, O(), "the options are null")
    go(I(), P(), None, "the output struct is null")
    go(I(table=None), P(), O(), "d_table is null")
    go(I(state=None), P(), O(), "d_state_in is null")
    go(I(), P(), O(state=None), "d_state_out is null")
    go(I(), P(), O(mask=None), "d_mask is null")
    go(I(ids=None), P(), O(), "d_ids is null")
    go(I(), P(n_words=nw - 1), O(), "n_words is too small")
    go(I(), P(n_words=(1 << 26) + 1), O(), "n_words is above 2^26")
    go(I(), P(8), O(), "unknown flag bit")
    go(I(), P(1 << 31), O(), "unknown flag bit")
    o = P()
    o.n_end = 9
    go(I(), o, O(), "n_end is above SPL_CHOICE_MAX_END")
    go(I(), P(end=()), O(), "no sequence could ever finish")
    go(I(), P(end=(3, 32 * nw)), O(), "at or above 32 * n_words")
    go(I(), P(ref.THEN_FREE, end=(32 * nw,)), O(), "at or above 32 * n_words")
    go(I(), P(), O(mask=ids.data_ptr()), "coincides with an input")
    go(I(), P(), O(live=tab.data_ptr()), "coincides with an input")
    go(I(), P(), O(mask=st.data_ptr()), "coincides with an input")
    go(I(), P(), O(live=lens.data_ptr()), "coincides with an input")
    go(I(), P(), O(mask=st2.data_ptr()), "coincides with d_state_out")
    go(I(ids=ids.data_ptr() + 4), P(ref.I64), O(), "not aligned")
    go(I(), P(), O(mask=mask.data_ptr() + 2), "not 4-byte aligned")
    go(I(state=st.data_ptr() + 4), P(), O(), "not 8-byte aligned")
    for which in range(3):
        si, o, so = I(), P(), O()
        (si, o, so)[which].struct_size = 8
        go(si, o, so, "struct_size")
    big = _ffi.SplChoiceIn((1 << 31), 0, None, None, st.data_ptr(), tab.data_ptr())
    go(big, P(), O(), "n_seqs >= 2^31")
    # state out with state in is the one overlap allowed; THEN_FREE needs no END id
    assert L.spl_choice_step_device(tok.handle, ctypes.byref(I()), ctypes.byref(P(ref.THEN_FREE, end=())), ctypes.byref(O(state=st.data_ptr())), None) == 0
    torch.cuda.synchronize()
    assert L.spl_set_option(tok.handle, b"choice_piece_words", 6) == -1 and L.spl_set_option(tok.handle, b"choice_piece_words", 8196) == -1
    assert L.spl_set_option(tok.handle, b"choice_piece_words", 0) == -1
    v = ctypes.c_int64()
    assert L.spl_get_option(tok.handle, b"choice_piece_words", ctypes.byref(v)) == 0 and v.value == 8192
    assert L.spl_set_option(tok.handle, b"choice_piece_words", 12) == 0 and L.spl_get_option(tok.handle, b"choice_piece_words", ctypes.byref(v)) == 0 and v.value == 12
    assert L.spl_set_option(tok.handle, b"choice_piece_words", 8192) == 0
    # the Python layer: dtypes, shapes, sizes
    with pytest.raises(ValueError, match="int32 or int64"):
        dv.choice_step_device(tok, ids.to(torch.int16), None, st, tab, end_ids=[4])
    with pytest.raises(ValueError, match="no sequence could ever finish"):
        dv.choice_step_device(tok, ids, None, st, tab)
    with pytest.raises(ValueError, match="at most 8"):
        dv.choice_step_device(tok, ids, None, st, tab, end_ids=list(range(9)))
    with pytest.raises(ValueError, match="at or above 32"):
        dv.choice_step_device(tok, ids, None, st, tab, end_ids=[32 * nw], n_words=nw)
    with pytest.raises(ValueError, match="n_words is too small"):
        dv.choice_step_device(tok, ids, None, st, tab, end_ids=[4], n_words=nw - 1)
    with pytest.raises(ValueError, match="keep_free needs"):
        dv.choice_step_device(tok, ids, None, st, tab, end_ids=[4], keep_free=True)
    with pytest.raises(ValueError, match=r"shape \[4160\]"):
        dv.choice_step_device(tok, ids, None, st, tab[:100], end_ids=[4])
    with pytest.raises(ValueError, match=r"shape \[batch, 2\]"):
        dv.choice_step_device(tok, ids, None, st[:, :1].contiguous(), tab, end_ids=[4])
    with pytest.raises(ValueError, match="1 .. 64 bytes"):
        dv.choice_table(["ok", ""])
    with pytest.raises(ValueError, match="1 .. 64 bytes"):
        dv.choice_table([b"x" * 65])
    with pytest.raises(ValueError, match="at most 64 choices"):
        dv.choice_table(["c%d" % i for i in range(65)])
    with pytest.raises(ValueError, match="slots are 0 .. 1"):
        dv.choice_state([[2]], 2)
    assert dv.choice_state([None, [], [1]], 2, dev).cpu().tolist() == [[3, 0], [0, 0], [2, 0]]


# ---------------------------------------------------------------------------------------------- the shipped vocabularies, end to end
LABELS = [" yes", " no", "yes", "no", "positive", "negative", "neutral", " positive", " negative", "A", "B", "C", "D", "true", "false",
          "get_weather", "get_time", "search_web", " maybe", "unknown", "Yes", "No", "yes.", "yesterday"]


def _matrix(tok):
    """(ids [n], bytes [n, 64] zero padded and cut, lengths [n], {id: bytes}, a special id) of a shipped vocabulary's ordinary tokens"""
    from splintr_amd import _ffi
    toks, special = [], None
    for i in range(tok.vocab_size):
        p, n = ctypes.c_void_p(), ctypes.c_uint32()
        kind = _ffi.lib().spl_token_bytes(tok.handle, i, ctypes.byref(p), ctypes.byref(n))
        if kind in (1, 2) and n.value:
            toks.append((i, ctypes.string_at(p, n.value)))
        elif kind == 3 and special is None:
            special = i
    M = np.zeros((len(toks), 64), dtype=np.uint8)
    for r, (_, b) in enumerate(toks):
        M[r, :min(len(b), 64)] = np.frombuffer(b[:64], dtype=np.uint8)
    return np.array([i for i, _ in toks], dtype=np.int64), M, np.array([len(b) for _, b in toks], dtype=np.int64), dict(toks), special


def _np_prefix_ids(ids, M, lens, r):
    """brute force: the ordinary ids whose bytes r starts with (|b(t)| <= |r|)"""
    if not r:
        return ids[:0]
    x = np.frombuffer(r[:64], dtype=np.uint8)
    eq = M[:, :len(x)] == x
    lead = np.where(eq.all(1), len(x), (~eq).argmax(1))                        # bytes shared at the front
    return ids[(lens <= len(r)) & (lead >= lens)]


@pytest.mark.parametrize("name", ["cl100k_base", "o200k_base", "deepseek_v3"])
def test_shipped_vocabulary_end_to_end(name):
    from splintr_amd import Tokenizer, corpus
    tok = Tokenizer.from_pretrained(name)
    ids, M, lens, by_id, special = _matrix(tok)
    assert special is not None
    words = []
    for t in corpus.c2(40):
        for w in t.split():
            if w.isascii() and w.isalpha() and 3 <= len(w) <= 12 and w not in words and w not in LABELS:
                words.append(w)
    choices = [c.encode() for c in (LABELS + words)[:64]]
    assert len(choices) == 64
    B, nw = 256, (tok.vocab_size + 31) // 32 + 3
    end = (special, 32 * nw - 1)
    rng = random.Random(17)
    sel = [None, [0], [63], list(range(0, 64, 2))] + [sorted(rng.sample(range(64), rng.choice([1, 2, 4, 4, 8, 64]))) for _ in range(B - 4)]
    states = [ref.begin(choices, s) for s in sel]
    toks_all = list(by_id.items())
    cache = {}

    def want_ids(st):
        out = []
        for s in st[0]:
            key = (s, st[1])
            if key not in cache:
                cache[key] = _np_prefix_ids(ids, M, lens, choices[s][st[1]:])
            out.append(cache[key])
        if any(len(choices[s]) == st[1] for s in st[0]):
            out.append(np.array(end, dtype=np.int64))
        return np.unique(np.concatenate(out))

    r = _call(tok, ref.table(choices), ids=cases.NO_IDS(B), state=cases.rows(states), end_ids=end, n_words=nw)
    drawn = [b""] * B
    for step in range(65):
        assert r["state"].tolist() == cases.rows(states).tolist(), (name, step)
        live = [b for b in range(B) if states[b][0]]
        assert r["live"].tolist() == [int(bool(s[0])) for s in states]
        if not live:
            break
        feed = np.zeros((B, 1), dtype=np.int64)
        ln = np.zeros(B, dtype=np.int32)
        for b in range(B):
            if not states[b][0]:
                assert (r["mask"][b] == 0xFFFFFFFF).all()
                continue
            ok = want_ids(states[b])
            row = np.zeros(nw, dtype=np.uint32)
            np.bitwise_or.at(row, ok >> 5, (np.uint32(1) << (ok & 31).astype(np.uint32)))
            assert (r["mask"][b] == row).all(), (name, step, b, states[b])
            t = int(ok[rng.randrange(len(ok))])                                  # the sampler: uniform over the row
            feed[b, 0], ln[b] = t, 1
            drawn[b] += by_id.get(t, b"")                                        # (an END id is no ordinary id here: it spells nothing)
            states[b] = ref.step(toks_all, choices, states[b], [t], end)
        r = _call(tok, ref.table(choices), ids=feed, lengths=ln, state=r["state"], end_ids=end, n_words=nw, in_place=True)
    assert all(s[3] and not s[2] for s in states), "a sequence is not done after 65 steps"
    for b, s in enumerate(states):
        assert s[4] in (sel[b] if sel[b] is not None else range(64)) and drawn[b] == choices[s[4]], (b, s, drawn[b])
    assert (r["mask"].view(np.int32) == -1).all()


# ---------------------------------------------------------------------------------------------- ChoiceGuide beside the streaming decode
def test_choice_guide_with_stream_decode_and_utf8_mask():
    import torch
    from splintr_amd import Tokenizer
    tok = Tokenizer.from_pretrained("cl100k_base")
    choices = ["positive", "negative", "中立", "très bien", " yes", "否"]
    B = 8
    special = _matrix(tok)[4]
    guide = tok.choice_guide(B, choices, end_ids=[special])
    dec = tok.device_streaming_decoder(B, skip_special_tokens=True)
    sel = [None, [0], [1], [2], [3], [2, 5], [4, 5], []]
    assert guide.begin(sel) is guide.mask
    dev = guide.mask.device
    assert guide.live.cpu().tolist() == [1, 1, 1, 1, 1, 1, 1, 0] and (guide.mask[7] == -1).all().item()
    gen = torch.Generator(device="cpu").manual_seed(5)
    texts = [""] * B
    for step in range(70):
        if not guide.live.any().item():
            break
        dec.allowed_mask(guide.mask, and_into=True)                             # the UTF-8 rows ANDed into the guide's
        logits = torch.rand((B, tok.vocab_size), generator=gen).to(dev)
        before = logits.clone()
        guide.apply(logits, live_only=True)
        live = guide.live.cpu().numpy().astype(bool)
        pick = logits.argmax(1)
        mask = guide.mask.cpu().numpy().view(np.uint32)
        for b, t in enumerate(pick.cpu().tolist()):
            if live[b]:
                assert t < 32 * guide.n_words and (int(mask[b, t >> 5]) >> (t & 31)) & 1, (step, b, t)
            else:
                assert torch.equal(logits[b], before[b])
        lens = guide.live.to(torch.int32)                                       # sequences that are done draw nothing more
        out = dec.add_tokens(pick.to(torch.int32), lens)
        texts = [a + (o or "") for a, o in zip(texts, out)]
        guide.step(pick, lens)
        assert not dec.stalled.any().item(), "a sequence stalled"
    assert not guide.live.any().item() and not guide.broken.any().item()
    hit = guide.hit.cpu().tolist()
    assert guide.done.cpu().tolist() == [True] * 7 + [False] and hit[7] == -1
    for b in range(7):
        assert hit[b] in (sel[b] if sel[b] is not None else range(len(choices))) and texts[b] == choices[hit[b]], (b, hit[b], texts[b])
        assert int(guide.spelled[b].item()) == len(choices[hit[b]].encode())
    assert (guide.mask == -1).all().item()
    # rows begin again while the others keep their state; reset frees a row
    guide.begin([[4]], rows=[7])
    assert guide.live.cpu().tolist() == [0] * 7 + [1] and guide.done.cpu().tolist() == [True] * 7 + [False]
    guide.reset([7])
    assert guide.state.cpu().tolist()[7] == [0, 0] and (guide.mask[7] == -1).all().item()
    # then_free: done as soon as a choice is spelled out, no END id needed
    free = tok.choice_guide(2, [" yes", " no"], then_free=True)
    free.begin()
    yes = tok.encode(" yes")
    assert len(yes) == 1
    free.step(torch.tensor([yes[0], tok.encode("x")[0]], dtype=torch.int64, device=dev))
    assert free.done.cpu().tolist() == [True, False] and free.broken.cpu().tolist() == [False, True] and free.hit.cpu().tolist() == [0, -1]
