"""GPU tests (-m gpu): spl_stop_match_device -- stop strings over a bytes CSR in HBM, per-sequence match state and hold-back -- through the
C ABI against the whole-text oracle of tests/stop_ref.py, and end to end through DeviceStreamingDecoder(stop=...) for the shipped
vocabularies against the host streaming decoders' text and the same oracle."""
import ctypes
import itertools
import json
import os

import numpy as np
import pytest

import stop_ref as ref

pytestmark = pytest.mark.gpu

POISON = 0xA5
WORD_POISON = 0x5A5A5A5A5A5A5A5A
STOP_SETS = [[b"a"], [b"ab", b"b"], [b"abc", b"bc"], [b"ab", b"abc"], [b"abca", b"bcab"], [b"bc", b"abc", b"bc"]]
LONG = bytes(range(65, 65 + 64))

_tok = {}


def _handle():
    """any handle: the call uses it for its device and its scratch only"""
    if "t" not in _tok:
        from splintr_amd import Tokenizer
        _tok["t"] = Tokenizer.from_pretrained("cl100k_base")
    return _tok["t"]


def _option(name, value=None):
    from splintr_amd import _ffi
    L = _ffi.lib()
    if value is not None:
        assert L.spl_set_option(_handle().handle, name, value) == 0
    v = ctypes.c_int64(-1)
    assert L.spl_get_option(_handle().handle, name, ctypes.byref(v)) == 0
    return int(v.value)


def _call(data, off, state, tab, *, masks=None, final=None, flags=0, cap, in_cap=None, in_place=False):
    """One call through the C ABI with poisoned outputs -> (bytes below min(need, cap), offsets, hits, rows (numpy), need); asserts that
    nothing at or beyond min(need, cap) was written, and nothing behind the offsets, the hits and the state rows."""
    import torch
    from splintr_amd import _ffi
    dev = torch.device("cuda", 0)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    B = off.shape[0] - 1
    data = np.ascontiguousarray(data, dtype=np.uint8)
    t_in = torch.from_numpy(data).to(dev)
    t_off = torch.from_numpy(off.view(np.int64)).to(dev)
    t_tab = torch.from_numpy(np.ascontiguousarray(tab, dtype=np.uint8)).to(dev)
    t_mask = None if masks is None else torch.from_numpy(np.array(masks, dtype=np.uint64).view(np.int64)).to(dev)
    t_fin = None if final is None else torch.from_numpy(np.ascontiguousarray(final, dtype=np.uint8)).to(dev)
    rows_in = np.concatenate([np.asarray(state, dtype=np.uint64).reshape(B, ref.WORDS), np.full((1, ref.WORDS), WORD_POISON, dtype=np.uint64)])
    t_sin = torch.from_numpy(rows_in.view(np.int64)).to(dev)
    t_sout = t_sin if in_place else torch.full((B + 1, ref.WORDS), WORD_POISON, dtype=torch.int64, device=dev)
    t_bytes = torch.full(((cap + 15) // 16 * 16 + 64,), POISON, dtype=torch.uint8, device=dev)
    t_oo = torch.full((B + 2,), WORD_POISON, dtype=torch.int64, device=dev)
    t_hit = torch.full((B + 1,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    rc = _ffi.lib().spl_stop_match_device(_handle().handle, ptr(t_in), data.shape[0] if in_cap is None else in_cap, t_off.data_ptr(), B,
                                          t_tab.data_ptr(), ptr(t_mask), ptr(t_fin), flags, t_sin.data_ptr(), t_sout.data_ptr(),
                                          t_bytes.data_ptr(), cap, t_oo.data_ptr(), t_hit.data_ptr(),
                                          torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, _ffi.last_error()
    oo = t_oo.cpu().numpy().view(np.uint64)
    st = t_sout.cpu().numpy().view(np.uint64)
    hit = t_hit.cpu().numpy()
    raw = t_bytes.cpu().numpy()
    assert oo[B + 1] == WORD_POISON and (st[B] == WORD_POISON).all() and hit[B] == 0x5A5A5A5A, "written behind the offsets, hits or rows"
    need = int(oo[B])
    m = min(need, cap)
    assert (raw[m:] == POISON).all(), "written at or beyond min(need, capacity)"
    return raw[:m].tobytes(), oo[:B + 1].copy(), hit[:B].copy(), st[:B].copy(), need


def _drive(tab, feeds, *, masks=None, include=False, final_all=False, in_place=False):
    """feeds: per sequence a list of (data, final), one entry per call: every call against the oracle -- bytes, offsets, hits and rows bit
    for bit.  Returns per sequence (the concatenated output, the hit)."""
    B = len(feeds)
    seqs = [ref.Seq(ref.live_stops(tab, None if masks is None else masks[b]), include) for b in range(B)]
    state = np.zeros((B, ref.WORDS), dtype=np.uint64)
    outs = [b""] * B
    flags = (ref.INCLUDE if include else 0) | (ref.FINAL_ALL if final_all else 0)
    for c in range(len(feeds[0]) if B else 0):
        call = [feeds[b][c] for b in range(B)]
        data, off = ref.csr([d for d, _ in call])
        fin = None if final_all or not any(f for _, f in call) else np.array([1 if f else 0 for _, f in call], dtype=np.uint8)
        raw, oo, hit, state, need = _call(data, off, state, tab, masks=masks, final=fin, flags=flags, cap=int(off[-1]) + 64 * B + 16,
                                          in_place=in_place)
        want = ref.run_calls(seqs, [[(d, f or final_all) for d, f in call]])[0]
        assert need == len(want[0]) and raw == want[0], ("bytes", c)
        assert (oo == want[1]).all(), ("offsets", c)
        assert (hit == want[2]).all(), ("hits", c)
        bad = np.nonzero((state != want[3]).any(axis=1))[0]
        assert bad.size == 0, ("rows", c, bad[:4], state[bad[:1]], want[3][bad[:1]])
        o = oo.astype(np.int64)
        outs = [outs[b] + raw[o[b]:o[b + 1]] for b in range(B)]
    return outs, [q.hit for q in seqs]


def _texts6():
    return [b"".join(t) for k in range(7) for t in itertools.product([b"a", b"b", b"c"], repeat=k)]


def test_exhaustive_alphabet_as_one_batch():
    """every text of up to 6 bytes over {a, b, c} x 6 stop sets (slots 10 k .. of ONE table, a mask per sequence) as ONE batch of 6 558
    sequences, fed whole and one byte a step: the same text and hit either way"""
    texts = _texts6()
    slots, masks, feeds = [None] * 64, [], []
    for k, stops in enumerate(STOP_SETS):
        m = 0
        for i, s in enumerate(stops):
            slots[10 * k + i] = s
            m |= 1 << (10 * k + i)
        masks += [m] * len(texts)
        feeds += texts
    tab = ref.table(slots)
    assert len(feeds) == 6 * 1093
    whole = _drive(tab, [[(t, False)] for t in feeds], masks=masks)
    steps = _drive(tab, [[(t[i:i + 1], False) for i in range(6)] for t in feeds], masks=masks)
    assert whole == steps


def test_batch_sizes_and_the_two_launch_shapes():
    one = _option(b"stop_one_max")
    assert 0 < one <= 1024
    tab = ref.table([b"abc", b"bc"])
    texts = _texts6()[-700:]
    for n in sorted({1, one - 1, one, one + 1, 300}):                  # (n_seqs = 0: test_an_empty_batch_in_both_forms)
        _drive(tab, [[(t[:3], False), (t[3:], False)] for t in texts[:n]])
    from splintr_amd import _ffi
    L = _ffi.lib()
    assert L.spl_set_option(_handle().handle, b"stop_one_max", 1025) == -1 and L.spl_set_option(_handle().handle, b"stop_one_max", -1) == -1
    assert _option(b"stop_one_max") == one


def test_an_empty_batch_in_both_forms():
    """n_seqs = 0 through the C ABI, one launch and three ("stop_one_max" 1024 and 0): rc 0, out_off[0] = 0, nothing else written
    (_call's poison checks); and through the Python wrapper, which passes substitute pointers for the empty state and hit tensors"""
    import torch
    from splintr_amd import device as dv
    one = _option(b"stop_one_max")
    tab = ref.table([b"ab"])
    try:
        for limit in (1024, 0):
            assert _option(b"stop_one_max", limit) == limit
            raw, oo, hit, rows, need = _call(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), np.zeros((0, ref.WORDS), dtype=np.uint64),
                                             tab, cap=32)
            assert raw == b"" and need == 0 and oo.tolist() == [0] and hit.shape == (0,) and rows.shape == (0, ref.WORDS)
            raw, oo, hit, rows, need = _call(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), np.zeros((0, ref.WORDS), dtype=np.uint64),
                                             tab, cap=0)
            assert need == 0 and oo.tolist() == [0]
            dev = torch.device("cuda", 0)
            out, off, hit, st = dv.stop_match_device(_handle(), torch.zeros(0, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int64, device=dev),
                                                     torch.zeros((0, ref.WORDS), dtype=torch.int64, device=dev), dv.stop_table(["ab"], dev), max_bytes=0)
            assert off.cpu().tolist() == [0] and hit.shape == (0,) and st.shape == (0, ref.WORDS)
    finally:
        _option(b"stop_one_max", one)


def test_every_option_reads_back_what_was_set():
    """spl_get_option against spl_set_option over every name of the header's list: set, get, and the first value again"""
    import re
    from conftest import ROOT
    from splintr_amd import Tokenizer, _ffi
    hdr = open(os.path.join(ROOT, "include", "splintr_hip.h")).read()
    block = hdr[hdr.index("/* Tuning switches"):hdr.index("int spl_set_option")]
    names = sorted(set(re.findall(r'"([a-z0-9_]+)"', block)) - {"memo_clear"})
    assert len(names) >= 28 and "stop_one_max" in names and "chunk_bytes" in names
    L = _ffi.lib()
    tok = Tokenizer.from_pretrained("cl100k_base")               # (a handle of its own: the options are the handle's; `tok` owns it
    h = tok.handle                                               #  and must outlive every call below)
    other = {"chunk_bytes": 1 << 20, "single_chunk_max_bytes": 1 << 20, "result_estimate_div": 3, "memo_bits": 12, "memo_long_bits": 8,
             "memo_log_cap": 64, "group_scan_min": 7, "range_tiles": 9, "fuse_max_tiles": 5, "copy_threads": 2, "decode_chunk_ids": 4096,
             "window_totals_chunk": 3, "stream_one_max": 17, "stop_one_max": 19}
    v = ctypes.c_int64()
    for n in names:
        assert L.spl_get_option(h, n.encode(), ctypes.byref(v)) == 0, n
        first = v.value
        new = other.get(n, (1 if first == 2 else 2) if n == "range_streams" else 1 - first)
        assert new != first, n
        assert L.spl_set_option(h, n.encode(), new) == 0, (n, new, _ffi.last_error())
        assert L.spl_get_option(h, n.encode(), ctypes.byref(v)) == 0 and v.value == new, (n, v.value, new)
        assert L.spl_set_option(h, n.encode(), first) == 0 and L.spl_get_option(h, n.encode(), ctypes.byref(v)) == 0 and v.value == first, n
    assert L.spl_get_option(h, b"no_such_option", ctypes.byref(v)) == -1 and L.spl_get_option(h, b"memo_clear", ctypes.byref(v)) == -1
    assert tok.handle == h


def test_one_size_through_both_forms():
    """the same 100 sequences through the one-launch and the three-launch form ("stop_one_max"): identical results"""
    one = _option(b"stop_one_max")
    tab = ref.table([b"abca", b"bcab", b"cc"])
    feeds = [[(t[:2], False), (t[2:], i % 3 == 0)] for i, t in enumerate(_texts6()[-100:])]
    res = []
    try:
        for limit in (1024, 0):
            assert _option(b"stop_one_max", limit) == limit
            res.append(_drive(tab, feeds))
    finally:
        _option(b"stop_one_max", one)
    assert res[0] == res[1]


def test_block_edges_and_the_top_of_the_one_launch_form():
    """three launches ("stop_one_max" 0) at the driver's block of 16 sequences, one either side of it and at two blocks plus one; one launch
    (1024) across the carry of its chunked LDS scan and at its last count slot: each against the oracle, and every size through the other
    form too with identical results"""
    import stop_sim
    g = stop_sim.geometry()
    assert g["seq_block"] == 16 and g["one_cap"] == 1024
    one = _option(b"stop_one_max")
    tab = ref.table([b"abca", b"bcab", b"cc"])
    texts = _texts6()[-1024:]
    sizes = {0: (1, 15, 16, 17, 32, 33), 1024: (65, 1023, 1024)}
    res = {}
    try:
        for limit in sizes:
            assert _option(b"stop_one_max", limit) == limit
            for n in sizes[0] + sizes[1024]:
                res[limit, n] = _drive(tab, [[(t[:2], False), (t[2:], i % 3 == 0)] for i, t in enumerate(texts[:n])])
    finally:
        _option(b"stop_one_max", one)
    for n in sizes[0] + sizes[1024]:
        assert res[0, n] == res[1024, n], n


def test_200_bytes_a_step_with_a_64_byte_stop_across_the_edges():
    """200 new bytes a sequence in one step; the 64-byte stop straddles the chunk edges (64, 128, 192) and the step edge"""
    tab = ref.table([LONG, b"zz"])
    feeds, want = [], []
    for shift in list(range(0, 137, 3)) + [63, 64, 65, 127, 128, 129, 136]:
        text = (b"." * shift + LONG + b"." * 400)[:400]
        feeds.append([(text[:200], False), (text[200:], False)])
        want.append(b"." * shift)
    for shift in range(137, 200, 2):                         # the stop begins in the first step and ends in the second
        text = (b"." * shift + LONG + b"." * 400)[:400]
        feeds.append([(text[:200], False), (text[200:], False)])
        want.append(b"." * shift)
    outs, hits = _drive(tab, feeds)
    assert outs == want and hits == [0] * len(feeds)
    # 63 bytes held, then a mismatch: they leave at once
    text = b"." * 137 + LONG[:63]
    outs, hits = _drive(tab, [[(text, False), (b"!", False)]] * 70)
    assert outs == [text + b"!"] * 70 and hits == [-1] * 70


def test_masks_final_subset_and_sticky():
    tab = ref.table([b"ab", b"bc", b"c", b"a", b"b"], lens={3: 0, 4: 65})
    texts = [b"xabcx", b"xabcx", b"xabcx", b"xabcx", b"xabcx", b"aabb"] * 20
    masks = [0b00001, 0b00010, 0b00100, 0b11000, 0, 0xFFFFFFFFFFFFFFFF] * 20
    outs, hits = _drive(tab, [[(t, False), (b"", True), (b"abc", False)] for t in texts], masks=masks)
    # (sequences 3 and 4 have no live stop: the final releases everything, and the "abc" fed behind it leaves too)
    assert outs[:6] == [b"x", b"xa", b"xab", b"xabcxabc", b"xabcxabc", b"a"] and hits[:6] == [0, 1, 2, -1, -1, 0]
    tab = ref.table([b"abc"])
    feeds = [[(t, i % 4 in (0, 2)), (b"c", False), (b"", False), (b"abc", True)] for i, t in enumerate([b"xxab", b"xxab", b"ab", b"xabc"] * 25)]
    outs, hits = _drive(tab, feeds)
    assert outs[:4] == [b"xxabc", b"xx", b"abc", b"x"] and hits[:4] == [0, 0, 0, 0]
    outs, hits = _drive(tab, [f[:1] for f in feeds], final_all=True)
    assert outs[:4] == [b"xxab", b"xxab", b"ab", b"x"] and hits[:4] == [-1, -1, -1, 0]
    outs, hits = _drive(tab, [f[:2] for f in feeds], include=True)
    assert outs[:4] == [b"xxabc", b"xxabc", b"abc", b"xabc"] and hits[:4] == [-1, 0, -1, 0]


def test_capacity_cuts_the_bytes_never_the_state():
    tab = ref.table([b"abc", b"bc"])
    texts = _texts6()
    for n in (50, len(texts)):
        data, off = ref.csr(texts[-n:])
        zero = np.zeros((n, ref.WORDS), dtype=np.uint64)
        raw, oo, hit, rows, need = _call(data, off, zero, tab, cap=1 << 16)
        assert need == len(raw) and need > 100
        for cap in (0, 1, 17, need - 1, need):
            r2, o2, h2, s2, n2 = _call(data, off, zero, tab, cap=cap)
            assert r2 == raw[:cap] and n2 == need and (o2 == oo).all() and (h2 == hit).all() and (s2 == rows).all(), cap


def test_state_out_may_be_state_in():
    tab = ref.table([b"abca", b"bcab"])
    for n in (60, 700):                                      # the one-launch and the three-launch form
        feeds = [[(t[:3], False), (t[3:], False)] for t in _texts6()[-n:]]
        assert _drive(tab, feeds, in_place=True) == _drive(tab, feeds)


def test_input_offsets_beyond_the_capacity_are_clamped():
    tab = ref.table([b"ab"])
    data = np.frombuffer(b"xxayyab!POISONPOISON", dtype=np.uint8).copy()
    off = np.array([0, 3, 5, 100, 2 ** 40], dtype=np.uint64)
    zero = np.zeros((4, ref.WORDS), dtype=np.uint64)
    raw, oo, hit, rows, _ = _call(data, off, zero, tab, cap=64, in_cap=8)
    assert raw == b"xxyy" and oo.tolist() == [0, 2, 4, 4, 4] and hit.tolist() == [-1, -1, 0, -1] and rows[3].tolist() == [0] * 10
    raw, oo, hit, rows, _ = _call(data, off, zero, tab, cap=64, in_cap=0)
    assert raw == b"" and (rows == 0).all() and hit.tolist() == [-1] * 4


def test_refusals():
    import torch
    from splintr_amd import _ffi
    L, h = _ffi.lib(), _handle().handle
    buf = torch.zeros(16384, dtype=torch.uint8, device="cuda")
    A = buf.data_ptr()                                       # (a region of its own for every argument)

    def call(t=h, inb=A, icap=64, ioff=A + 512, n=3, tab=A + 1024, fl=0, s_in=A + 5632, s_out=A + 6144, out=A + 6656, cap=64, oo=A + 7168,
             hit=A + 7680):
        return L.spl_stop_match_device(t, inb, icap, ioff, n, tab, None, None, fl, s_in, s_out, out, cap, oo, hit, None)

    for kw, word in ((dict(t=None), "null handle"), (dict(tab=None), "d_table"), (dict(s_in=None), "d_state_in"), (dict(s_out=None), "d_state_out"),
                     (dict(oo=None), "d_out_off"), (dict(hit=None), "d_hit"), (dict(ioff=None), "d_in_off"), (dict(inb=None), "d_in_bytes"),
                     (dict(out=None), "d_out_bytes"), (dict(out=A + 6664), "16-byte"), (dict(fl=4), "unknown stop_flags"),
                     (dict(n=1 << 31), "2^31")):
        assert call(**kw) == -1 and word in L.spl_last_error().decode(), kw
    assert call() == 0                                       # (three empty sequences of an all-zero table: nothing matches, nothing leaves)
    torch.cuda.synchronize()


STOPS = ["\n\n", "###", " the ", "。"]
EXTRA = ["first part\n\nsecond part", "a title ### and more", "one\ntwo\n\nthree ###", "句子一。句子二。", "over the hill", "no stop in here at all",
         "##\n#\n \n###", "the theme then the end", "ends with a held newline\n"]


@pytest.mark.parametrize("name", ["cl100k_base", "o200k_base", "deepseek_v3"])
def test_shipped_vocabularies_end_to_end(name):
    """the fixture texts' ids through DeviceStreamingDecoder(stop=...) with K = 1 and K = 3: every step's released text is the oracle's for
    the host streaming decoder's text; both K give the same concatenated text and hit; `finished` stays a device tensor"""
    import torch
    from conftest import ROOT
    from splintr_amd import Tokenizer, _ffi
    with open(os.path.join(ROOT, "tests", "golden", "reference_test_strings.json"), encoding="utf-8") as f:
        texts = json.load(f)["plain"] + EXTRA
    tok = Tokenizer.from_pretrained(name)
    ids = tok.encode_batch(texts)
    B = len(texts)
    byte_level = bool(_ffi.lib().spl_is_byte_level(tok.handle))
    tab = ref.table(STOPS)
    results = []
    for K in (1, 3):
        host = [tok.byte_level_streaming_decoder() if byte_level else tok.streaming_decoder() for _ in texts]
        seqs = [ref.Seq(ref.live_stops(tab)) for _ in texts]
        dec = tok.device_streaming_decoder(B, stop=STOPS)
        steps = (max(len(x) for x in ids) + K - 1) // K
        got = [""] * B
        for k in range(steps):
            rows = np.zeros((B, K), dtype=np.int64)
            lens = np.zeros(B, dtype=np.int32)
            piece = []
            for b, x in enumerate(ids):
                part = x[k * K:(k + 1) * K]
                rows[b, :len(part)] = part
                lens[b] = len(part)
                piece.append("".join(host[b].add_token(i) or "" for i in part))
            out = dec.add_tokens(torch.from_numpy(rows).cuda(), torch.from_numpy(lens).cuda())
            want = [seqs[b].feed(piece[b].encode("utf-8")).decode("utf-8") or None for b in range(B)]
            assert out == want, (name, K, k, [(b, out[b], want[b]) for b in range(B) if out[b] != want[b]][:3])
            got = [g + (o or "") for g, o in zip(got, out)]
            fin = dec.finished
            assert isinstance(fin, torch.Tensor) and fin.is_cuda and fin.dtype == torch.bool and fin.shape == (B,)
            assert dec.stop_hit.is_cuda and dec.stop_hit.dtype == torch.int32
        assert dec.stop_hit.cpu().tolist() == [q.hit for q in seqs] and dec.finished.cpu().tolist() == [q.hit >= 0 for q in seqs]
        tail = dec.flush()
        want = [seqs[b].feed(b"", True).decode("utf-8") or None for b in range(B)]
        assert tail == want
        got = [g + (o or "") for g, o in zip(got, tail)]
        results.append((got, dec.stop_hit.cpu().tolist()))
        # against the definition on the whole text
        for b, t in enumerate(texts):
            f = ref.first_hit(t.encode("utf-8"), ref.live_stops(tab))
            assert got[b] == (t.encode("utf-8")[:f[1]].decode("utf-8") if f else t), (name, K, b)
    assert results[0] == results[1]
    assert sum(h >= 0 for h in results[0][1]) >= 6 and sum(h < 0 for h in results[0][1]) >= 6


def test_device_streaming_decoder_with_stops(monkeypatch):
    """the repeat on a short buffer keeps both kept states; set_stop_mask, reset, include_stop_str_in_output; stop=None has no stop surface"""
    import torch
    tok = _handle()
    text = ["alpha ### beta", "no stop here, but a long line that does not fit sixteen bytes", "x\n\ny", ""]
    ids = tok.encode_batch(text)
    K = max(map(len, ids))
    rows = np.zeros((4, K), dtype=np.int64)
    lens = np.array([len(x) for x in ids], dtype=np.int32)
    for b, x in enumerate(ids):
        rows[b, :len(x)] = x
    d_rows, d_lens = torch.from_numpy(rows).cuda(), torch.from_numpy(lens).cuda()
    dec = tok.device_streaming_decoder(4, stop=["###", "\n\n"])
    dec.BYTES_PER_ID = 0                                     # the first buffer is 16 bytes: both calls are repeated from the kept states
    assert dec.add_tokens(d_rows, d_lens) == ["alpha ", text[1], "x", None]
    assert dec.stop_hit.cpu().tolist() == [0, -1, 1, -1] and dec.finished.cpu().tolist() == [True, False, True, False]
    # step_device alone: a decode buffer that is too short is signalled on the device, and a large enough one is not
    probe = tok.device_streaming_decoder(4, stop=["###", "\n\n"])
    probe.step_device(d_rows, d_lens, max_bytes=16)
    assert probe.decode_overflowed.is_cuda and probe.decode_overflowed.item() and probe.decode_need.item() == sum(len(t.encode()) for t in text)
    probe.reset()
    probe.step_device(d_rows, d_lens)
    assert not probe.decode_overflowed.item() and probe.decode_need.item() == sum(len(t.encode()) for t in text)
    assert dec.add_tokens(d_rows, d_lens) == [None, text[1], None, None]           # finished sequences stay silent
    dec.reset(rows=[0])
    dec.set_stop_mask([0], 0b10)                             # sequence 0: only "\n\n" applies
    assert dec.add_tokens(d_rows, d_lens)[0] == text[0] and dec.stop_hit.cpu().tolist()[0] == -1
    dec.reset()
    assert (dec.stop_state == 0).all().item() and not dec.finished.any().item()
    inc = tok.device_streaming_decoder(4, stop=["###", "\n\n"], include_stop_str_in_output=True)
    assert inc.add_tokens(d_rows, d_lens) == ["alpha ###", text[1], "x\n\n", None]
    plain = tok.device_streaming_decoder(4)
    assert plain.add_tokens(d_rows, d_lens) == [text[0], text[1], text[2], None]
    with pytest.raises(ValueError, match="stop"):
        plain.finished
