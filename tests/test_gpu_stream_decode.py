"""GPU tests (-m gpu): spl_stream_decode_device -- one step of B streaming decoders per call, state in HBM -- against the two oracles of
tests/stream_ref.py (the host StreamingDecoder for hold mode, Python's incremental decoder for replace mode) and, for the shipped
vocabularies, against the host streaming decoders step for step."""
import ctypes

import numpy as np
import pytest

import stream_ref as ref
import vocabgen

pytestmark = pytest.mark.gpu

I64, SKIP_SPECIAL = 1, 4
POISON = 0xA5
MODES = pytest.mark.parametrize("replace", [False, True], ids=["hold", "replace"])

_tok = {}


def _byte_tok():
    """tests/stream_ref.byte_table as a handle: 256 single-byte keys and two long ones, built the way test_gpu_vocab_generated.py builds its
    vocabularies; the literals are special tokens"""
    if "bytes" not in _tok:
        from splintr_amd import CL100K_BASE_PATTERN, Tokenizer
        tab = ref.byte_table()
        enc = {v: k for k, v in tab.tokens.items() if k not in tab.special_only}
        special = {tab.tokens[k].decode("utf-8"): k for k in tab.special_only}
        _tok["bytes"] = Tokenizer.from_bytes(vocabgen.tiktoken(enc), CL100K_BASE_PATTERN, special)
    return _tok["bytes"]


def _one_max():
    import stream_sim
    return stream_sim.geometry()["one_max"]


def _call(tok, rows, lens, state, *, replace, flags=0, final=None, final_all=False, cap, in_place=False):
    """One call through the C ABI with poisoned outputs -> (bytes below min(need, cap), offsets, state_out (numpy uint64), need); asserts
    that nothing at or beyond min(need, cap) was written, and nothing behind the offsets and the state words."""
    import torch
    from splintr_amd import _ffi
    dev = torch.device("cuda", 0)
    rows = np.ascontiguousarray(rows)
    assert rows.dtype == (np.int64 if flags & I64 else np.uint32)
    B, K = rows.shape
    t_rows = torch.from_numpy(rows.view(np.int64 if flags & I64 else np.int32)).to(dev)
    t_len = None if lens is None else torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).to(dev)
    t_fin = None if final is None else torch.from_numpy(np.ascontiguousarray(final, dtype=np.uint8)).to(dev)
    t_in = torch.from_numpy(np.concatenate([np.asarray(state, dtype=np.uint64), [np.uint64(0x5A5A5A5A5A5A5A5A)]]).view(np.int64)).to(dev)
    t_out = t_in if in_place else torch.full((B + 1,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    t_bytes = torch.full(((cap + 15) // 16 * 16 + 64,), POISON, dtype=torch.uint8, device=dev)
    t_off = torch.full((B + 2,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    o = _ffi.SplDecodeOpts(flags, K)
    sflags = (ref.REPLACE if replace else 0) | (ref.FINAL_ALL if final_all else 0)
    rc = _ffi.lib().spl_stream_decode_device(tok.handle, ptr(t_rows), ptr(t_len), B, ctypes.byref(o), sflags, ptr(t_fin), t_in.data_ptr(),
                                             t_out.data_ptr(), t_bytes.data_ptr(), cap, t_off.data_ptr(),
                                             torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, _ffi.last_error()
    off = t_off.cpu().numpy()
    st = t_out.cpu().numpy().view(np.uint64)
    raw = t_bytes.cpu().numpy()
    assert off[B + 1] == 0x5A5A5A5A5A5A5A5A and st[B] == 0x5A5A5A5A5A5A5A5A, "written behind the offsets or the state words"
    need = int(off[B])
    m = min(need, cap)
    assert (raw[m:] == POISON).all(), "written at or beyond min(need, capacity)"
    return raw[:m].tobytes(), off[:B + 1], st[:B].copy(), need


def _slice(res, n):
    return res[0][:n], res[1][:n], res[2][:n]


def _run_steps(tok, n, replace):
    """the first n alphabet strings one byte per step, four steps and a final one, against the shared oracle"""
    strings = ref.alphabet_strings()[:n]
    rows, lens = ref.rows_of(strings)
    want = ref.alphabet_oracle(replace, "steps")
    state = np.zeros(n, dtype=np.uint64)
    for k in range(4):
        raw, off, state, need = _call(tok, rows[:, k:k + 1], (lens > k).astype(np.int32), state, replace=replace, cap=6 * n + 16)
        ref.check_step(("steps", n, replace, k), raw, off, state, _slice(want[k], n))
    raw, off, state, _ = _call(tok, rows[:, :1], np.zeros(n, dtype=np.int32), state, replace=replace, final_all=True, cap=6 * n + 16)
    ref.check_step(("steps", n, replace, "final"), raw, off, state, _slice(want[4], n))


@MODES
def test_exhaustive_alphabet_as_one_batch(replace):
    """every string of up to four bytes over the 15-byte alphabet as ONE batch of 54 240 sequences, K = 1; shorter strings idle (len 0)"""
    _run_steps(_byte_tok(), 54240, replace)


@MODES
def test_batch_sizes_and_the_two_launch_shapes(replace):
    one = _one_max()
    for n in sorted({1, 63, 64, 65, 257, one - 1, one, one + 1}):
        _run_steps(_byte_tok(), n, replace)


def test_both_shapes_at_one_size():
    """the same 100 sequences through the one-launch and the three-launch form ("stream_one_max")"""
    from splintr_amd import _ffi
    tok = _byte_tok()
    L = _ffi.lib()
    try:
        for limit in (0, 99, 100, _one_max()):
            assert L.spl_set_option(tok.handle, b"stream_one_max", limit) == 0
            _run_steps(tok, 100, True)
    finally:
        assert L.spl_set_option(tok.handle, b"stream_one_max", _one_max()) == 0
    import stream_sim
    cap = stream_sim.geometry()["one_cap"]
    assert L.spl_set_option(tok.handle, b"stream_one_max", cap + 1) == -1 and L.spl_set_option(tok.handle, b"stream_one_max", -1) == -1


@MODES
def test_block_edges_and_the_top_of_the_one_launch_form(replace):
    """three launches ("stream_one_max" 0) at the driver's block of 16 sequences, one either side of it and at two blocks plus one; one launch
    (1024) across the carry of its chunked LDS scan and at its last count slot"""
    import stream_sim
    from splintr_amd import _ffi
    g = stream_sim.geometry()
    assert g["seq_block"] == 16 and g["one_cap"] == 1024
    tok, L = _byte_tok(), _ffi.lib()
    try:
        for limit, sizes in ((0, (1, 15, 16, 17, 32, 33)), (1024, (65, 1023, 1024))):
            assert L.spl_set_option(tok.handle, b"stream_one_max", limit) == 0
            for n in sizes:
                _run_steps(tok, n, replace)
    finally:
        assert L.spl_set_option(tok.handle, b"stream_one_max", _one_max()) == 0


def _random_rows(rng, B, K):
    pool = list(range(256)) * 3 + list(ref.CH2 + ref.CH3 + ref.CH4) * 40 + [ref.KEY4, ref.KEY2, ref.LIT3, ref.SPECIAL, ref.FAR] * 8 + \
        list(ref.UNKNOWN) * 6
    return rng.choice(np.array(pool, dtype=np.int64), size=(B, K))


@MODES
@pytest.mark.parametrize("K", [5, 70])
def test_rows_of_several_ids(K, replace):
    """[B, K], both dtypes: ragged len (below 0 and beyond K among them), int64 rows with negative padding and values beyond 32 bits,
    SKIP_SPECIAL; two steps, the second from the first one's state.  K = 70 takes a second window of slots."""
    rng = np.random.default_rng(K)
    tab, tok, B = ref.byte_table(), _byte_tok(), 150
    for flags in (0, I64, I64 | SKIP_SPECIAL, SKIP_SPECIAL):
        bt = ref.Batch(tab, B, flags, replace)
        state = np.zeros(B, dtype=np.uint64)
        for step in range(2):
            rows = _random_rows(rng, B, K)
            lens = rng.integers(-1, K + 3, size=B).astype(np.int32)
            lens[:4] = [0, K, K + 50, 1]
            if flags & I64:
                odd = rng.random((B, K)) < 0.05
                rows[odd] = rng.choice([-1, -100, 1 << 32, (1 << 32) + 0x41], size=int(odd.sum()))
                for b in range(B):
                    rows[b, min(max(int(lens[b]), 0), K):] = -100                  # what a collator leaves behind a row's ids
            r = rows if flags & I64 else rows.astype(np.uint32)
            want = bt.step(rows, None if step else lens)
            need = sum(len(w) for w in want[0])
            raw, off, state, got_need = _call(tok, r, None if step else lens, state, replace=replace, flags=flags, cap=need)
            assert got_need == need
            ref.check_step(("rows", K, flags, step), raw, off, state, want)


@MODES
def test_long_tokens_straddle_chunk_edges(replace):
    rows, lens = ref.straddle_rows()
    tab, tok = ref.byte_table(), _byte_tok()
    for flags in (0, I64):
        bt = ref.Batch(tab, len(rows), flags, replace)
        state = np.zeros(len(rows), dtype=np.uint64)
        for step in range(2):
            want = bt.step(rows, lens)
            raw, off, state, need = _call(tok, rows if flags else rows.astype(np.uint32), lens, state, replace=replace, flags=flags, cap=1 << 16)
            ref.check_step(("straddle", flags, step), raw, off, state, want)


TEXTS = ["Hello, world!", "你好世界", "Hello 🌍 World!", "naïve café", "日本語のテキスト", "한국어 텍스트", "🙂🙃😀😃😄", "a", "", "Привет, мир",
         "emoji 👨‍👩‍👧‍👦 family", "tab\tand\nnewline", "数字 12345 と記号 !?", "ß ü ö ä", "👍🏽 skin tone", "mixed 中文 and English",
         "العربية", "עברית", "ไทย", "हिन्दी", "🇩🇪🇯🇵", "x" * 40, "汉" * 20, "😀" * 9, "α β γ δ"]


def _texts():
    out = list(TEXTS)
    i = 0
    while len(out) < 65:
        out.append(TEXTS[i % len(TEXTS)] + " " + TEXTS[(i * 7 + 3) % len(TEXTS)][::-1])
        i += 1
    return out[:65]


@pytest.mark.parametrize("name", ["cl100k_base", "o200k_base", "deepseek_v3"])
def test_shipped_vocabularies_step_for_step(name):
    """65 short texts with CJK and emoji, encoded by this tokenizer and fed back one id per step through DeviceStreamingDecoder: every step
    equals the host streaming decoder of the vocabulary's kind, and the concatenation is the text"""
    import torch
    from splintr_amd import Tokenizer, _ffi
    tok = Tokenizer.from_pretrained(name)
    texts = _texts()
    ids = tok.encode_batch(texts)
    byte_level = bool(_ffi.lib().spl_is_byte_level(tok.handle))
    host = [tok.byte_level_streaming_decoder() if byte_level else tok.streaming_decoder() for _ in texts]
    dec = tok.device_streaming_decoder(len(texts))
    steps = max(len(x) for x in ids)
    rows = np.zeros((len(texts), steps), dtype=np.int64)
    for b, x in enumerate(ids):
        rows[b, :len(x)] = x
    lens = np.array([len(x) for x in ids])
    d_rows = torch.from_numpy(rows).cuda()
    got = [""] * len(texts)
    for k in range(steps):
        live = torch.from_numpy((lens > k).astype(np.int32)).cuda()
        out = dec.add_tokens(d_rows[:, k].contiguous(), live)
        want = [host[b].add_token(ids[b][k]) if k < len(ids[b]) else None for b in range(len(texts))]
        assert out == want, (name, k, [(b, out[b], want[b]) for b in range(len(texts)) if out[b] != want[b]][:3])
        got = [g + (o or "") for g, o in zip(got, out)]
        assert dec.pending_bytes.cpu().tolist() == [h.pending_bytes for h in host], (name, k)
    assert got == texts
    assert not dec.stalled.any().item() and dec.flush() == [None] * len(texts)


@MODES
def test_capacity_cuts_the_bytes_never_the_state(replace):
    rows, lens = ref.straddle_rows()
    rows = rows.astype(np.uint32)
    tok = _byte_tok()
    zero = np.zeros(len(rows), dtype=np.uint64)
    raw, off, state, need = _call(tok, rows, lens, zero, replace=replace, cap=1 << 16)
    assert need == len(raw) and need > 1000
    for cap in (0, 1, 17, need - 1, need):
        r2, o2, s2, n2 = _call(tok, rows, lens, zero, replace=replace, cap=cap)
        assert r2 == raw[:cap] and n2 == need and o2.tolist() == off.tolist() and s2.tolist() == state.tolist(), cap


@MODES
def test_state_out_may_be_state_in(replace):
    tok = _byte_tok()
    for n in (100, 1500):                     # the one-launch and the three-launch form
        strings = ref.alphabet_strings()[-n:]
        rows, lens = ref.rows_of(strings)
        s_a = s_b = np.zeros(n, dtype=np.uint64)
        for cut in ((0, 2), (2, 4)):
            part = rows[:, cut[0]:cut[1]]
            ra, oa, s_a, _ = _call(tok, part, None, s_a, replace=replace, cap=16 * n)
            rb, ob, s_b, _ = _call(tok, part, None, s_b, replace=replace, cap=16 * n, in_place=True)
            assert ra == rb and oa.tolist() == ob.tolist() and s_a.tolist() == s_b.tolist()


@MODES
def test_final_for_a_subset(replace):
    """d_final for every third sequence: those flush, the others go on unchanged and finish their character in the next step"""
    tab, tok, B = ref.byte_table(), _byte_tok(), 300
    bt = ref.Batch(tab, B, 0, replace)
    first = np.tile(np.array([[0x41, ref.CH4[0], ref.CH4[1]]], dtype=np.uint32), (B, 1))
    first[1::2] = [0x42, 0x43, ref.CH3[0]]
    rest = np.tile(np.array([[ref.CH4[2], ref.CH4[3], 0x5A]], dtype=np.uint32), (B, 1))
    rest[1::2] = [ref.CH3[1], ref.CH3[2], 0x59]
    fin = (np.arange(B) % 3 == 0).astype(np.uint8)
    state = np.zeros(B, dtype=np.uint64)
    raw, off, state, _ = _call(tok, first, None, state, replace=replace, final=fin, cap=16 * B)
    ref.check_step(("final subset", 0), raw, off, state, bt.step(first, None, fin))
    assert [int(s) == 0 for s in state] == [bool(f) for f in fin]
    raw, off, state, _ = _call(tok, rest, None, state, replace=replace, cap=16 * B)
    ref.check_step(("final subset", 1), raw, off, state, bt.step(rest))
    assert raw[int(off[1]):int(off[2])] == ref.CH3 + b"Y" and raw[int(off[2]):int(off[3])] == ref.CH4 + b"Z"


def test_device_streaming_decoder_end_to_end(monkeypatch):
    """add_tokens with [B] and [B, K], the repeat on a short buffer, flush, reset, pending_bytes and stalled"""
    import torch
    from splintr_amd import device as dv
    sizes, plain = [], dv.stream_decode_device
    monkeypatch.setattr(dv, "stream_decode_device", lambda *a, **k: (sizes.append(k["max_bytes"]), plain(*a, **k))[1])
    tok = _byte_tok()
    text = ["héllo 你好 😀!", "plain", "😀😀😀😀😀😀😀😀", ""]
    data = [t.encode() for t in text]
    for errors in ("hold", "replace"):
        dec = tok.device_streaming_decoder(4, errors=errors)
        dec.BYTES_PER_ID = 0                                  # every step's first buffer is 16 bytes: the long row repeats
        K = 16
        got = [""] * 4
        for k0 in range(0, max(map(len, data)), K):
            rows = np.zeros((4, K), dtype=np.int32)
            lens = np.zeros(4, dtype=np.int32)
            for b, d in enumerate(data):
                part = d[k0:k0 + K]
                rows[b, :len(part)] = list(part)
                lens[b] = len(part)
            out = dec.add_tokens(torch.from_numpy(rows).cuda(), torch.from_numpy(lens).cuda())
            assert out[3] is None
            got = [g + (o or "") for g, o in zip(got, out)]
        assert got == text and dec.pending_bytes.cpu().tolist() == [0, 0, 0, 0]
        assert sizes[:2] == [16, 14 + 5 + 16], sizes             # the first step ran twice: 16 bytes, then the exact need (row 0 keeps two bytes)
        one = torch.tensor([0xF0, 0x41, 0x80, 0xE4], dtype=torch.int64).cuda()
        out = dec.add_tokens(one)
        assert out == ([None, "A", None, None] if errors == "hold" else [None, "A", "�", None])
        assert dec.stalled.cpu().tolist() == [False, False, errors == "hold", False]
        assert dec.pending_bytes.cpu().tolist() == [1, 0, 1 if errors == "hold" else 0, 1]
        assert dec.flush(rows=[0]) == ["�", None, None, None] and dec.pending_bytes.cpu().tolist()[3] == 1
        assert dec.flush() == [None, None, None, "�"]
        assert dec.stalled.cpu().tolist()[2] == (errors == "hold")
        dec.reset(rows=[2])
        assert not dec.stalled.any().item() and dec.add_tokens(one[[1, 1, 1, 1]].contiguous()) == ["A"] * 4
        dec.reset()
        assert dec.state.cpu().tolist() == [0, 0, 0, 0]
