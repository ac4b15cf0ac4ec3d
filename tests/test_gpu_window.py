"""GPU tests (-m gpu) of spl_window_device (csrc/spl_k_window.h): the CSR as overlapping windows of every document.

Expected values: tests/window_ref.py (plain loops, written from the header's semantics); end to end the ids come from the oracle.
As in test_gpu_collate.py every output the kernels write is a view INSIDE one allocation with 64 guard elements in front and behind it,
filled with a sentinel like the view itself: each check asserts that the guards are untouched; an element the kernel skipped shows as the
sentinel in the comparison with the expected values.  Shapes are tiny: rows of 1..65 entries, at most a few thousand documents.  A
capacity below the need is a defined outcome (d_n reports the need, nothing beyond the capacity is written), not a fault."""
import ctypes

import numpy as np
import pytest

import window_ref as ref
from window_ref import BOS, EOS, I64, PAD_LEFT
from test_gpu_parity import tok

pytestmark = pytest.mark.gpu

NAME = "cl100k_base"
LS = [1, 2, 3, 4, 5, 7, 8, 63, 64, 65]
GUARD = 64
PAD_ID, BOS_ID, EOS_ID = 0xFFFFFFFF, 0x80000001, 0xFFFFFFFD          # bit patterns that a sign extension would show
SENT = {"int32": 0x5A5A5A5A, "int64": 0x5A5A5A5A5A5A5A5A, "uint8": 0x5A}
SCAN_SPAN = 4096                                                     # documents per workgroup of the scan (WIN_SPAN)


def _dev():
    import torch
    return torch.device("cuda", 0)


class Guarded:
    """numel elements between two guards of GUARD elements, one allocation, all of it the sentinel (test_gpu_collate.py's, restated)"""

    def __init__(self, numel, dtype):
        import torch
        self.sent = SENT[str(dtype).split(".")[-1]]
        self.whole = torch.full((numel + 2 * GUARD,), self.sent, dtype=dtype, device=_dev())
        self.numel = numel

    def ptr(self):
        return self.whole.data_ptr() + GUARD * self.whole.element_size()

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


def _want(ids, off, L, flags, overlap):
    return ref.window_ref(ids, off, L, flags & ~I64, overlap, PAD_ID, BOS_ID, EOS_ID)


def _same_ids(got, want64, i64):
    if i64:
        return np.array_equal(got.view(np.uint64), want64)            # int64 rows hold the ZERO-extended 32 bits
    return np.array_equal(got.view(np.uint32), want64.astype(np.uint32))


NULLABLE = ("mask", "len", "doc", "start")


def _win(t, d_ids, d_off, n_docs, L, flags, overlap, want, rows_cap, null=None):
    """one spl_window_device call into guarded buffers of rows_cap rows, compared with want = window_ref(...)"""
    import torch
    from splintr_amd import _ffi
    lib = _ffi.lib()
    i64 = bool(flags & I64)
    w_rows, w_mask, w_len, w_doc, w_start, w_off = want
    need = len(w_len)
    rows = Guarded(rows_cap * L, torch.int64 if i64 else torch.int32)
    mask = Guarded(rows_cap * L, torch.uint8)
    lens = Guarded(rows_cap, torch.int32)
    doc = Guarded(rows_cap, torch.int32)
    start = Guarded(rows_cap, torch.int64)
    roff = Guarded(n_docs + 1, torch.int64)
    dn = Guarded(2, torch.int64)
    words = lib.spl_window_work_bytes(n_docs) // 8
    work = Guarded(words, torch.int64)
    o = _opts(L, flags)
    rc = lib.spl_window_device(t.handle, d_ids.data_ptr(), d_off.data_ptr(), n_docs, ctypes.byref(o), overlap, rows.ptr(), rows_cap,
                               None if null == "mask" else mask.ptr(), None if null == "len" else lens.ptr(),
                               None if null == "doc" else doc.ptr(), None if null == "start" else start.ptr(), roff.ptr(), dn.ptr(),
                               work.ptr() if words else None, _stream())
    assert rc == 0, _ffi.last_error()
    tag = (n_docs, L, flags, overlap, rows_cap, null)
    work.host()
    assert dn.host().tolist() == [need, min(need, rows_cap)], tag      # the NEED, whatever the cap
    assert np.array_equal(roff.host().view(np.uint64), w_off), tag     # complete, whatever the cap
    m = min(need, rows_cap)
    r = rows.host()
    assert _same_ids(r[:m * L], w_rows.reshape(-1)[:m * L], i64), tag
    assert _same_ids(r[m * L:], np.full((rows_cap - m) * L, PAD_ID, np.uint64), i64), tag
    for name, buf, full, rest in (("mask", mask, w_mask.reshape(-1)[:m * L], 0), ("len", lens, w_len[:m], 0), ("doc", doc, w_doc[:m], -1),
                                  ("start", start, w_start[:m], 0)):
        h = buf.host()
        if null == name:
            assert (h == buf.sent).all(), tag + (name,)
        else:
            assert np.array_equal(h[:len(full)], full) and (h[len(full):] == rest).all(), tag + (name,)


# ------------------------------------------------------------------------------------------ 1. synthetic CSR, every path of the gather
@pytest.mark.parametrize("L", LS)
def test_window_synthetic(L):
    t = tok(NAME)
    rng = np.random.default_rng(300 + L)
    first = True
    for base in (0, BOS, EOS, BOS | EOS, PAD_LEFT, PAD_LEFT | BOS | EOS):
        B = L - ref.n_special(base)
        if B < 1:                                     # (refused: no room for a token)
            continue
        for overlap in ref.overlaps(B):
            edges = ref.edge_lengths(B, B - overlap)
            for n_docs in (1, 2, 301):
                lens = [edges[i] for i in rng.integers(0, len(edges), size=n_docs)] if n_docs > 1 else [edges[-1]]
                ids, off = ref.csr(lens, rng)
                d_ids, d_off = _upload(ids, off)
                want = _want(ids, off, L, base, overlap)
                need = len(want[2])
                for flags in (base, base | I64):      # both dtypes against ONE reference; one row more than needed: it holds padding
                    _win(t, d_ids, d_off, n_docs, L, flags, overlap, want, rows_cap=need + 1)
                if n_docs == 301:
                    _win(t, d_ids, d_off, n_docs, L, base | (I64 if L & 1 else 0), overlap, want, rows_cap=need)
                    _win(t, d_ids, d_off, n_docs, L, base, overlap, want, rows_cap=need - 1)      # one row short: d_n still reports the need
                    _win(t, d_ids, d_off, n_docs, L, base | I64, overlap, want, rows_cap=need // 2)
                    _win(t, d_ids, d_off, n_docs, L, base, overlap, want, rows_cap=0)
                    for null in NULLABLE if first else ():        # each optional output NULL in turn
                        _win(t, d_ids, d_off, n_docs, L, base | (I64 if null in ("len", "start") else 0), overlap, want, rows_cap=need + 1, null=null)
                    first = False
    assert not first


def test_no_documents_and_one_empty_document():
    t = tok(NAME)
    for lens in ([], [0]):
        ids, off = ref.csr(lens)
        d_ids, d_off = _upload(ids, off)
        for L, flags in ((1, 0), (5, BOS | EOS | I64), (64, PAD_LEFT | EOS)):
            want = _want(ids, off, L, flags, 0)
            assert len(want[2]) == len(lens)
            for cap in (0, 1, 3):
                _win(t, d_ids, d_off, len(lens), L, flags, 0, want, rows_cap=cap)


def test_scalar_tail_of_the_flat_output():
    """rows_cap * L no multiple of 4: the last lane's group is partial and stores element by element"""
    t = tok(NAME)
    rng = np.random.default_rng(31)
    for L, n_docs in ((7, 151), (5, 1), (3, 343), (65, 17)):
        ids, off = ref.csr(rng.integers(0, 3 * L, size=n_docs).tolist(), rng)
        d_ids, d_off = _upload(ids, off)
        want = _want(ids, off, L, BOS, 1 if L > 2 else 0)
        need = len(want[2])
        for cap in (need, need + 1, need + 2, need + 3):
            if (cap * L) % 4:
                _win(t, d_ids, d_off, n_docs, L, BOS | (I64 if cap & 1 else 0), 1 if L > 2 else 0, want, rows_cap=cap)


def test_one_document_whose_windows_fill_several_spans():
    t = tok(NAME)
    rng = np.random.default_rng(32)
    for L, flags, overlap, n_ids in ((3, BOS, 1, 5000), (4, I64, 3, 7000), (9, BOS | EOS | PAD_LEFT, 0, 30000), (65, EOS, 63, 4000)):
        ids, off = ref.csr([2, n_ids, 0, 1], rng)
        d_ids, d_off = _upload(ids, off)
        want = _want(ids, off, L, flags, overlap)
        need = len(want[2])
        assert need * L > 3 * 1024                    # more than three spans of the gather
        _win(t, d_ids, d_off, 4, L, flags, overlap, want, rows_cap=need)
        _win(t, d_ids, d_off, 4, L, flags, overlap, want, rows_cap=need - 7)


# ------------------------------------------------------------------------------------------ 2. every level of the scan
@pytest.mark.parametrize("n_docs", [SCAN_SPAN - 1, SCAN_SPAN, SCAN_SPAN + 1, 2 * SCAN_SPAN + 1])
def test_scan_levels(n_docs):
    """one launch up to the scan's span, three beyond it; with "window_totals_chunk" at 2 (and 1) the three spans of 2 span + 1 documents
    take two (three) rounds of the second launch.  Random lengths, empties among them; L = 1 fills every gather window with documents."""
    from splintr_amd import _ffi
    t = tok(NAME)
    lib = _ffi.lib()
    assert (lib.spl_window_work_bytes(n_docs) == 0) == (n_docs <= SCAN_SPAN)
    rng = np.random.default_rng(n_docs)
    try:
        for L, flags, overlap, top in ((1, 0, 0, 2), (4, BOS | I64, 1, 12), (7, BOS | EOS | PAD_LEFT, 4, 12)):
            lens = rng.integers(0, top, size=n_docs).tolist()
            lens[0] = lens[-1] = 0
            ids, off = ref.csr(lens, rng)
            d_ids, d_off = _upload(ids, off)
            want = _want(ids, off, L, flags, overlap)
            need = len(want[2])
            for chunk in ((256, 2, 1) if n_docs > 2 * SCAN_SPAN else (256,)):
                assert lib.spl_set_option(t.handle, b"window_totals_chunk", chunk) == 0
                _win(t, d_ids, d_off, n_docs, L, flags, overlap, want, rows_cap=need + 1)
            _win(t, d_ids, d_off, n_docs, L, flags, overlap, want, rows_cap=need // 3)
    finally:
        assert lib.spl_set_option(t.handle, b"window_totals_chunk", 256) == 0
    assert lib.spl_set_option(t.handle, b"window_totals_chunk", 0) == -1 and lib.spl_set_option(t.handle, b"window_totals_chunk", 257) == -1


# ------------------------------------------------------------------------------------------ 3. end to end
def _texts():
    from splintr_amd import corpus
    return ["", "Hello, world!", "你好世界", "Hello 🌍 World!"] + corpus.c2(16) + corpus.c3(1, doc_bytes=6144)


def _csr_of(lists):
    off = np.zeros(len(lists) + 1, dtype=np.uint64)
    if lists:
        off[1:] = np.cumsum([len(x) for x in lists])
    return np.array([x for l in lists for x in l], dtype=np.uint32), off


@pytest.mark.parametrize("name", ["cl100k_base", "deepseek_v3"])
def test_end_to_end(coracle, name):
    """real texts through encode_device: windows equal to window_ref over the oracle's ids; Tokenizer.encode_batch_windows agrees"""
    import torch
    from splintr_amd.device import DeviceBatch, encode_device, window_device
    t = tok(name)
    texts = _texts()
    ids, off = _csr_of(coracle(name).encode_batch(texts))
    n = len(texts)
    st = torch.cuda.Stream(device=_dev())
    with torch.cuda.stream(st):                       # encode and windows queued on ONE non-default stream, nothing in between
        b = DeviceBatch(texts, _dev())
        b.ids.fill_(0x5A5A5A5A)
        encode_device(t, b)
        w32 = window_device(t, b, 32, overlap=8, pad_id=PAD_ID, bos_id=BOS_ID, eos_id=EOS_ID)
        w64 = window_device(t, b, 33, overlap=0, pad_id=PAD_ID, eos_id=EOS_ID, padding_side="left", dtype=torch.int64)
        small = window_device(t, b, 32, overlap=8, pad_id=PAD_ID, bos_id=BOS_ID, eos_id=EOS_ID, max_rows=5)
    st.synchronize()
    for got, L, flags, overlap, i64 in ((w32, 32, BOS | EOS, 8, False), (w64, 33, EOS | PAD_LEFT, 0, True), (small, 32, BOS | EOS, 8, False)):
        want = ref.window_ref(ids, off, L, flags, overlap, PAD_ID, BOS_ID, EOS_ID)
        need, cap = len(want[2]), got[0].shape[0]
        m = min(need, cap)
        assert need > n and (cap >= need or got is small)
        assert got[6].cpu().tolist() == [need, m]
        assert got[0].shape == (cap, L) and got[1].dtype == torch.uint8 and got[2].dtype == torch.int32 and got[3].dtype == torch.int32
        assert got[4].dtype == torch.int64 and got[5].dtype == torch.int64 and got[5].shape == (n + 1,)
        assert _same_ids(got[0][:m].cpu().numpy().reshape(-1), want[0][:m].reshape(-1), i64)
        assert np.array_equal(got[1][:m].cpu().numpy(), want[1][:m]) and np.array_equal(got[2][:m].cpu().numpy(), want[2][:m])
        assert np.array_equal(got[3][:m].cpu().numpy(), want[3][:m]) and np.array_equal(got[4][:m].cpu().numpy(), want[4][:m])
        assert np.array_equal(got[5].cpu().numpy().view(np.uint64), want[5])
        assert (got[0][m:].cpu().numpy().view(np.uint64 if i64 else np.uint32) == PAD_ID).all() and (got[3][m:] == -1).all()
        assert (got[1][m:] == 0).all() and (got[2][m:] == 0).all() and (got[4][m:] == 0).all()
    for L, overlap, kw, flags in ((24, 5, dict(bos_id=1), BOS), (40, 0, dict(eos_id=2, padding_side="left", dtype=torch.int64), EOS | PAD_LEFT)):
        rows, mask, lens, doc, start, row_off = t.encode_batch_windows(texts, L, overlap=overlap, pad_id=7, **kw)
        want = ref.window_ref(ids, off, L, flags, overlap, 7, 1, 2)
        assert rows.shape == (len(want[2]), L) and rows.device.type == "cuda" and mask.shape == rows.shape
        assert _same_ids(rows.cpu().numpy().reshape(-1), want[0].reshape(-1), rows.dtype == torch.int64)
        assert np.array_equal(mask.cpu().numpy(), want[1]) and np.array_equal(lens.cpu().numpy(), want[2])
        assert np.array_equal(doc.cpu().numpy(), want[3]) and np.array_equal(start.cpu().numpy(), want[4])
        assert np.array_equal(row_off.cpu().numpy().view(np.uint64), want[5])
    rows, mask, lens, doc, start, row_off = t.encode_batch_windows([], 8, pad_id=0)
    assert rows.shape == (0, 8) and row_off.cpu().tolist() == [0]
    with pytest.raises(ValueError, match="overlap"):
        t.encode_batch_windows(texts, 8, pad_id=0, overlap=8)


def test_round_trip_through_the_device_decode():
    """overlap 0 and no BOS / EOS: the windows of a document, decoded row by row and joined in row_off order, are the document's bytes"""
    from splintr_amd import device as dv
    t = tok(NAME)
    texts = _texts()
    b = dv.DeviceBatch(texts, _dev())
    dv.encode_device(t, b)
    for L, side in ((16, "right"), (37, "left")):
        rows, mask, lens, doc, start, row_off, n = dv.window_device(t, b, L, overlap=0, pad_id=9906, padding_side=side)     # (the pad id would decode)
        out, off = dv.decode_rows_device(t, rows, lens, max_bytes=b.n_bytes, padding_side=side)
        o_h, raw, r_off = off.cpu().tolist(), out.cpu().numpy().tobytes(), row_off.cpu().tolist()
        assert int(n[0]) == r_off[-1] <= rows.shape[0] and o_h[-1] == b.n_bytes
        for d, text in enumerate(texts):
            assert raw[o_h[r_off[d]]:o_h[r_off[d + 1]]] == text.encode("utf-8"), (L, side, d)
