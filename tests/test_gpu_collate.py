"""GPU tests (-m gpu) of spl_pad_device / spl_pack_device (csrc/spl_k_collate.h): the CSR as a padded batch and as packed sequences.

Expected values: tests/collate_ref.py (plain loops, written from the header's semantics); end to end the ids come from the oracle.
Every output the kernels write is a view INSIDE one allocation with 64 guard elements in front and behind it, filled with a sentinel
like the view itself: each check asserts that the guards are untouched; an element the kernel skipped shows as the sentinel in the
comparison with the expected values.  Shapes are tiny: rows of 1..65 entries, at most a few thousand documents."""
import ctypes

import numpy as np
import pytest

import collate_ref as ref
from collate_ref import BOS, EOS, I64, KEEP_TAIL, PAD_LEFT
from test_gpu_parity import tok

pytestmark = pytest.mark.gpu

NAME = "cl100k_base"
LS = [1, 2, 3, 4, 5, 7, 8, 63, 64, 65]
GUARD = 64
PAD_ID, BOS_ID, EOS_ID = 0xFFFFFFFF, 0x80000001, 0xFFFFFFFD          # bit patterns that a sign extension would show
SENT = {"int32": 0x5A5A5A5A, "int64": 0x5A5A5A5A5A5A5A5A, "uint8": 0x5A}


def _dev():
    import torch
    return torch.device("cuda", 0)


class Guarded:
    """numel elements between two guards of GUARD elements, one allocation, all of it the sentinel"""

    def __init__(self, numel, dtype):
        import torch
        self.sent = SENT[str(dtype).split(".")[-1]]
        self.whole = torch.full((numel + 2 * GUARD,), self.sent, dtype=dtype, device=_dev())
        self.view = self.whole[GUARD:GUARD + numel]
        self.numel = numel

    def ptr(self):
        return self.view.data_ptr() if self.numel else self.whole.data_ptr() + GUARD * self.whole.element_size()

    def host(self):
        """the view on the host; the guards must still hold the sentinel"""
        w = self.whole.cpu().numpy()
        assert (w[:GUARD] == self.sent).all() and (w[GUARD + self.numel:] == self.sent).all(), "a guard was written"
        return w[GUARD:GUARD + self.numel]


def _upload(ids, off):
    import torch
    d_ids = torch.from_numpy(np.concatenate([ids, np.zeros(1, np.uint32)]).view(np.int32)).to(_dev())      # (never a null pointer)
    d_off = torch.from_numpy(off.astype(np.int64)).to(_dev())
    return d_ids, d_off


def _stream():
    import torch
    return torch.cuda.current_stream(_dev()).cuda_stream


def _opts(L, flags):
    from splintr_amd import _ffi
    return _ffi.SplCollateOpts(flags, L, PAD_ID, BOS_ID if flags & BOS else 0x11111111, EOS_ID if flags & EOS else 0x22222222)


def _same_ids(got, want64, i64):
    if i64:
        return np.array_equal(got.view(np.uint64), want64)            # int64 rows hold the ZERO-extended 32 bits
    return np.array_equal(got.view(np.uint32), want64.astype(np.uint32))


def _pad(t, d_ids, d_off, n_docs, L, flags, want, null=None):
    """one spl_pad_device call into guarded buffers, compared with want = (rows, mask, lens)"""
    import torch
    from splintr_amd import _ffi
    i64 = bool(flags & I64)
    rows = Guarded(n_docs * L, torch.int64 if i64 else torch.int32)
    mask = Guarded(n_docs * L, torch.uint8)
    lens = Guarded(n_docs, torch.int32)
    o = _opts(L, flags)
    rc = _ffi.lib().spl_pad_device(t.handle, d_ids.data_ptr(), d_off.data_ptr(), n_docs, ctypes.byref(o), rows.ptr(),
                                   None if null == "mask" else mask.ptr(), None if null == "len" else lens.ptr(), _stream())
    assert rc == 0, _ffi.last_error()
    tag = (n_docs, L, flags, null)
    assert _same_ids(rows.host(), want[0].reshape(-1), i64), tag
    m, ln = mask.host(), lens.host()
    assert (m == SENT["uint8"]).all() if null == "mask" else np.array_equal(m, want[1].reshape(-1)), tag
    assert (ln == SENT["int32"]).all() if null == "len" else np.array_equal(ln, want[2]), tag


def _pack(t, d_ids, d_off, n_docs, L, flags, want, rows_cap, null=None):
    """one spl_pack_device call into guarded buffers of rows_cap rows, compared with want = pack_ref(...)"""
    import torch
    from splintr_amd import _ffi
    i64 = bool(flags & I64)
    w_rows, w_doc, w_pos, n_rows, S = want
    rows = Guarded(rows_cap * L, torch.int64 if i64 else torch.int32)
    doc = Guarded(rows_cap * L, torch.int32)
    pos = Guarded(rows_cap * L, torch.int32)
    dn = Guarded(2, torch.int64)
    o = _opts(L, flags)
    rc = _ffi.lib().spl_pack_device(t.handle, d_ids.data_ptr(), d_off.data_ptr(), n_docs, ctypes.byref(o), rows.ptr(), rows_cap,
                                    None if null == "doc" else doc.ptr(), None if null == "pos" else pos.ptr(), dn.ptr(), _stream())
    assert rc == 0, _ffi.last_error()
    tag = (n_docs, L, flags, rows_cap, null)
    assert dn.host().tolist() == [n_rows, S], tag                      # the NEED, whatever the cap
    m = min(n_rows, rows_cap) * L                                      # elements the stream reaches below the cap
    r, d, p = rows.host(), doc.host(), pos.host()
    assert _same_ids(r[:m], w_rows.reshape(-1)[:m], i64), tag
    assert _same_ids(r[m:], np.full(rows_cap * L - m, PAD_ID, np.uint64), i64), tag
    if null == "doc":
        assert (d == SENT["int32"]).all(), tag
    else:
        assert np.array_equal(d[:m], w_doc.reshape(-1)[:m]) and (d[m:] == -1).all(), tag
    if null == "pos":
        assert (p == SENT["int32"]).all(), tag
    else:
        assert np.array_equal(p[:m], w_pos.reshape(-1)[:m]) and (p[m:] == 0).all(), tag


# ------------------------------------------------------------------------------------------ 4. pad, synthetic CSR
@pytest.mark.parametrize("L", LS)
def test_pad_synthetic(L):
    t = tok(NAME)
    rng = np.random.default_rng(100 + L)
    for n_docs in (1, 2, 257, 1025):
        for base in range(0, 32, 2):                  # every combination of PAD_LEFT, KEEP_TAIL, BOS, EOS ...
            k = ref.n_special(base)
            if L < k:                                 # (refused: row_len < BOS + EOS)
                continue
            ids, off = ref.csr(ref.sweep_lengths(L, k, n_docs, rng), rng)
            d_ids, d_off = _upload(ids, off)
            want = ref.pad_ref(ids, off, L, base, PAD_ID, BOS_ID, EOS_ID)
            for flags in (base, base | I64):          # ... with both dtypes, against ONE reference
                _pad(t, d_ids, d_off, n_docs, L, flags, want)
            if base == (BOS | PAD_LEFT) and n_docs == 257:
                _pad(t, d_ids, d_off, n_docs, L, base, want, null="mask")
                _pad(t, d_ids, d_off, n_docs, L, base | I64, want, null="len")


def test_pad_refusals_and_empty_batch():
    """what test_collate_cpu.py checks with a dummy handle, once with a real one; and n_docs = 0 (nothing is written)"""
    import torch
    from splintr_amd import _ffi
    t = tok(NAME)
    d_ids, d_off = _upload(np.zeros(0, np.uint32), np.zeros(1, np.uint64))
    rows = Guarded(0, torch.int32)
    o = _opts(4, 0)
    assert _ffi.lib().spl_pad_device(t.handle, d_ids.data_ptr(), d_off.data_ptr(), 0, ctypes.byref(o), rows.ptr(), None, None, _stream()) == 0
    rows.host()
    assert _ffi.lib().spl_pad_device(t.handle, d_ids.data_ptr(), d_off.data_ptr(), 1, ctypes.byref(_opts(1, BOS | EOS)), rows.ptr(), None, None,
                                     _stream()) == -1
    assert "BOS + EOS" in _ffi.last_error()


# ------------------------------------------------------------------------------------------ 5. pack, synthetic CSR
def _pack_shapes(L, k):
    fill = max(1, -(-(k + 1) // L) + 1) * L - k       # one document whose piece of the stream is a whole number of rows
    return {
        "three_rows": [1, 3 * L + 2, 2],
        "one_token_docs": [1] * 5000,
        "empty_runs": [0] * 5000 + [3] + [0] * 5000 + [4] + [0] * 5000,
        "all_empty": [0] * 50,
        "exact_multiple": [fill],
        "no_docs": [],
    }


@pytest.mark.parametrize("shape", ["three_rows", "one_token_docs", "empty_runs", "all_empty", "exact_multiple", "no_docs"])
def test_pack_synthetic(shape):
    t = tok(NAME)
    rng = np.random.default_rng(200)
    first = True
    for L in LS:
        for base in (0, BOS, EOS, BOS | EOS):         # k = 0, 1, 1, 2
            k = ref.n_special(base)
            lens = _pack_shapes(L, k)[shape]
            ids, off = ref.csr(lens, rng)
            d_ids, d_off = _upload(ids, off)
            want = ref.pack_ref(ids, off, L, base, PAD_ID, BOS_ID, EOS_ID)
            n_rows, S = want[3], want[4]
            if shape == "exact_multiple":
                assert S and S % L == 0
            if shape == "no_docs" or (shape == "all_empty" and k == 0):
                assert S == 0 and n_rows == 0
            for flags in (base, base | I64):
                _pack(t, d_ids, d_off, len(lens), L, flags, want, rows_cap=n_rows + 1)       # one row more than needed: it holds padding
            _pack(t, d_ids, d_off, len(lens), L, base | (I64 if L & 1 else 0), want, rows_cap=n_rows)
            if n_rows:
                _pack(t, d_ids, d_off, len(lens), L, base, want, rows_cap=n_rows - 1)          # one row short: d_n still reports the need
                _pack(t, d_ids, d_off, len(lens), L, base | I64, want, rows_cap=0)
            if first or (L == 65 and base == BOS):
                _pack(t, d_ids, d_off, len(lens), L, base, want, rows_cap=n_rows + 1, null="doc")
                _pack(t, d_ids, d_off, len(lens), L, base | I64, want, rows_cap=n_rows + 1, null="pos")
                first = False


# ------------------------------------------------------------------------------------------ 6. end to end, in stream order
def _texts():
    from splintr_amd import corpus
    return ["", "Hello, world!", "你好世界", "Hello 🌍 World!"] + corpus.c2(16) + corpus.c3(1, doc_bytes=6144)


def _csr_of(lists):
    off = np.zeros(len(lists) + 1, dtype=np.uint64)
    if lists:
        off[1:] = np.cumsum([len(x) for x in lists])
    return np.array([x for l in lists for x in l], dtype=np.uint32), off


@pytest.mark.parametrize("special", [False, True])
def test_end_to_end_stream_order(coracle, special):
    import torch
    from splintr_amd import _ffi
    from splintr_amd.device import DeviceBatch, encode_device, pack_device, pad_device
    t = tok(NAME)
    texts = _texts()
    eot = t._special["<|endoftext|>"]
    if special:
        texts = texts + ["one<|endoftext|>two <|endoftext|>", "<|endoftext|>"]
    ids, off = _csr_of(coracle(NAME).encode_batch(texts, special))
    if special:
        assert (ids == eot).sum() == 3
    n = len(texts)
    bos, eos = (None, eot) if special else (BOS_ID, EOS_ID)
    fl = EOS if special else BOS | EOS
    o_ids = (0x11111111 if bos is None else bos, eos)
    w_pad = ref.pad_ref(ids, off, 32, fl, PAD_ID, o_ids[0], o_ids[1])
    st = torch.cuda.Stream(device=_dev())
    with torch.cuda.stream(st):                       # encode, pad and pack queued on ONE non-default stream, nothing in between
        b = DeviceBatch(texts, _dev())
        b.ids.fill_(0x5A5A5A5A)
        encode_device(t, b, special)
        p32 = pad_device(t, b, 32, pad_id=PAD_ID, bos_id=bos, eos_id=eos)
        p64 = pad_device(t, b, 33, pad_id=PAD_ID, bos_id=bos, eos_id=eos, padding_side="left", truncation_side="left", dtype=torch.int64)
        k32 = pack_device(t, b, 128, pad_id=PAD_ID, bos_id=bos, eos_id=eos)
        k64 = pack_device(t, b, 127, pad_id=PAD_ID, bos_id=bos, eos_id=eos, dtype=torch.int64)
        # and once through the C ABI into a guarded buffer, still on that stream
        rows = Guarded(n * 32, torch.int32)
        o = _ffi.SplCollateOpts(fl, 32, PAD_ID, o_ids[0], o_ids[1])
        assert _ffi.lib().spl_pad_device(t.handle, b.ids.data_ptr(), b.out_off.data_ptr(), n, ctypes.byref(o), rows.ptr(), None, None,
                                         st.cuda_stream) == 0
    st.synchronize()
    assert _same_ids(rows.host(), w_pad[0].reshape(-1), False)
    for got, L, flags, i64 in ((p32, 32, fl, False), (p64, 33, fl | PAD_LEFT | KEEP_TAIL, True)):
        want = ref.pad_ref(ids, off, L, flags, PAD_ID, o_ids[0], o_ids[1])
        assert got[0].shape == (n, L) and got[1].dtype == torch.uint8 and got[2].dtype == torch.int32
        assert _same_ids(got[0].cpu().numpy().reshape(-1), want[0].reshape(-1), i64)
        assert np.array_equal(got[1].cpu().numpy(), want[1]) and np.array_equal(got[2].cpu().numpy(), want[2])
    for got, L, i64 in ((k32, 128, False), (k64, 127, True)):
        want = ref.pack_ref(ids, off, L, fl, PAD_ID, o_ids[0], o_ids[1])
        n_rows, S = want[3], want[4]
        assert got[3].cpu().tolist() == [n_rows, S] and got[0].shape[0] >= n_rows
        assert _same_ids(got[0][:n_rows].cpu().numpy().reshape(-1), want[0].reshape(-1), i64)
        assert np.array_equal(got[1][:n_rows].cpu().numpy(), want[1]) and np.array_equal(got[2][:n_rows].cpu().numpy(), want[2])
        assert (got[0][n_rows:].cpu().numpy().view(np.uint64 if i64 else np.uint32) == PAD_ID).all() and (got[1][n_rows:] == -1).all()


# ------------------------------------------------------------------------------------------ 7. the convenience methods
def test_tokenizer_convenience_methods(coracle):
    import torch
    t = tok(NAME)
    texts = _texts()
    ids, off = _csr_of(coracle(NAME).encode_batch(texts))
    n = len(texts)
    for L in (16, 40):                                # twice on one handle, different lengths
        rows, mask, lens = t.encode_batch_padded(texts, L, pad_id=0, eos_id=100257, dtype=torch.int64)
        want = ref.pad_ref(ids, off, L, EOS, 0, 0, 100257)
        assert rows.shape == (n, L) and rows.dtype == torch.int64 and rows.device.type == "cuda"
        assert mask.shape == (n, L) and mask.dtype == torch.uint8 and lens.shape == (n,) and lens.dtype == torch.int32
        assert np.array_equal(rows.cpu().numpy().view(np.uint64), want[0])
        assert np.array_equal(mask.cpu().numpy(), want[1]) and np.array_equal(lens.cpu().numpy(), want[2])
    rows, mask, lens = t.encode_batch_padded(texts, 24, pad_id=7, bos_id=1, padding_side="left", truncation_side="left")
    want = ref.pad_ref(ids, off, 24, BOS | PAD_LEFT | KEEP_TAIL, 7, 1, 0)
    assert rows.dtype == torch.int32 and np.array_equal(rows.cpu().numpy().view(np.uint32), want[0].astype(np.uint32))
    assert np.array_equal(mask.cpu().numpy(), want[1])
    for L in (64, 200):
        rows, doc, pos = t.encode_batch_packed(texts, L, pad_id=0, bos_id=1, eos_id=2)
        want = ref.pack_ref(ids, off, L, BOS | EOS, 0, 1, 2)
        assert rows.shape == (want[3], L) and rows.dtype == torch.int32 and rows.device.type == "cuda"
        assert doc.shape == rows.shape and doc.dtype == torch.int32 and pos.shape == rows.shape and pos.dtype == torch.int32
        assert np.array_equal(rows.cpu().numpy().view(np.uint32), want[0].astype(np.uint32))
        assert np.array_equal(doc.cpu().numpy(), want[1]) and np.array_equal(pos.cpu().numpy(), want[2])
    rows, doc, pos = t.encode_batch_packed([], 8, pad_id=0)
    assert rows.shape == (0, 8)
    with pytest.raises(ValueError, match="dtype"):
        t.encode_batch_padded(texts, 8, pad_id=0, dtype=torch.int16)
    with pytest.raises(ValueError, match="dtype"):
        t.encode_batch_packed(texts, 8, pad_id=0, dtype=torch.float32)
    with pytest.raises(ValueError, match="padding_side"):
        t.encode_batch_padded(texts, 8, pad_id=0, padding_side="up")
    with pytest.raises(ValueError, match="truncation_side"):
        t.encode_batch_padded(texts, 8, pad_id=0, truncation_side="middle")
