"""GPU tests (-m gpu) of spl_pair_device (csrc/spl_k_pair.h): two CSRs joined into one row per pair of documents.

Expected values: tests/pair_ref.py (plain loops, written from the header's semantics; LONGEST_FIRST as the sequential rule); end to end
the ids come from the oracle.  The grid is test_pair_cpu.py's (pair_ref.grid).  Every output the kernel writes is a view INSIDE one
allocation with 64 guard elements in front and behind it, filled with a sentinel like the view itself (test_gpu_collate.Guarded): each
check asserts that the guards are untouched; an element the kernel skipped shows as the sentinel in the comparison.  Shapes are tiny:
rows of 1..130 entries, at most a few thousand pairs.  (Index arithmetic beyond 2^32 flat elements is covered by the host simulation
alone, test_pair_cpu.py: no memory holds such an output.)"""
import ctypes

import numpy as np
import pytest

import pair_ref as ref
from pair_ref import I64, KEEP_TAIL_A, KEEP_TAIL_B, LONGEST_FIRST, ONLY_FIRST, ONLY_SECOND, PAD_LEFT
from test_gpu_collate import SENT, Guarded, _dev, _same_ids, _stream
from test_gpu_parity import tok

pytestmark = pytest.mark.gpu

NAME = "cl100k_base"
PAD_ID = 0xFFFFFFFF
OUTPUTS = ("mask", "type", "special", "len", "kept")


def _upload(ids, off):
    import torch
    d_ids = torch.from_numpy(np.concatenate([ids, np.zeros(1, np.uint32)]).view(np.int32)).to(_dev())      # (never a null pointer)
    return d_ids, torch.from_numpy(off.astype(np.int64)).to(_dev())


def _index(idx):
    import torch
    return None if idx is None else torch.tensor(idx, dtype=torch.int32, device=_dev())


def _pair(t, dev_src, a_idx, b_idx, n_pairs, L, flags, trunc, segs, want, null=()):
    """one spl_pair_device call into guarded buffers, compared with want = pair_ref(...)"""
    import torch
    from splintr_amd import _ffi
    d_a_ids, d_a_off, n_a, d_b_ids, d_b_off, n_b = dev_src
    i64 = bool(flags & I64)
    rows = Guarded(n_pairs * L, torch.int64 if i64 else torch.int32)
    by = {n: Guarded(n_pairs * L, torch.uint8) for n in ("mask", "type", "special")}
    lens, kept, status = Guarded(n_pairs, torch.int32), Guarded(2 * n_pairs, torch.int32), Guarded(1, torch.int32)
    status.view.zero_()                               # (the one word the caller clears)
    ia, ib = _index(a_idx), _index(b_idx)
    o = _ffi.SplPairOpts(flags, L, PAD_ID, trunc, *segs)
    ptr = lambda name, g: None if name in null else g.ptr()
    rc = _ffi.lib().spl_pair_device(t.handle, d_a_ids.data_ptr(), d_a_off.data_ptr(), n_a, d_b_ids.data_ptr(), d_b_off.data_ptr(), n_b,
                                    None if ia is None else ia.data_ptr(), None if ib is None else ib.data_ptr(), n_pairs, ctypes.byref(o),
                                    rows.ptr(), ptr("mask", by["mask"]), ptr("type", by["type"]), ptr("special", by["special"]),
                                    ptr("len", lens), ptr("kept", kept), status.ptr(), _stream())
    assert rc == 0, _ffi.last_error()
    tag = (n_pairs, L, flags, trunc, tuple(map(len, segs)), null)
    assert _same_ids(rows.host(), want[0].reshape(-1), i64), tag
    for i, name, g in ((1, "mask", by["mask"]), (2, "type", by["type"]), (3, "special", by["special"]), (4, "len", lens), (5, "kept", kept)):
        got = g.host()
        if name in null:
            assert (got == g.sent).all(), (name,) + tag                     # not wanted: not written
        else:
            assert np.array_equal(got, want[i].reshape(-1)), (name,) + tag
    assert status.host().tolist() == [want[6]], tag


# ------------------------------------------------------------------------------------------ 1. the grid, synthetic CSRs
@pytest.mark.parametrize("L", ref.ROW_LENS + ref.LONG_ROW_LENS)
def test_pair_grid(L):
    t = tok(NAME)
    cases = 0
    for src, calls, _, flags, trunc, segs in ref.grid(L, 20260 + L):            # (test_pair_cpu.py's cases, seed for seed)
        a_ids, a_off, n_a, b_ids, b_off, n_b = src
        dev_src = _upload(a_ids, a_off) + (n_a,) + _upload(b_ids, b_off) + (n_b,)
        for kind, a_idx, b_idx, bad, n_pairs in calls:
            want = ref.pair_ref(a_ids, a_off, n_a, b_ids, b_off, n_b, a_idx, b_idx, n_pairs, L, flags, PAD_ID, trunc, *segs)
            assert want[6] == (1 if bad else 0)
            _pair(t, dev_src, a_idx, b_idx, n_pairs, L, flags | (I64 if cases & 1 else 0), trunc, segs, want)     # both dtypes, in alternation
            cases += 1
    assert cases >= 120


def test_pair_both_dtypes_optional_outputs_and_many_pairs():
    """a few thousand pairs -- more than one workgroup, rows that straddle lanes and workgroups -- in int32 and int64 against ONE
    reference; each optional output passed as NULL once (it stays sentinel), and all of them at once"""
    t = tok(NAME)
    rng = np.random.default_rng(20264)
    segs = ((0xA0000000,), (0xB0000000, 0xB0000001), (0xC0000000,))
    for n_docs, L in ((300, 65), (1025, 3), (2100, 5), (700, 64)):
        sg = segs if L >= 4 else ((), (), ())
        budget = L - sum(map(len, sg))
        a_ids, a_off = ref.csr(ref.sweep_lengths(budget, n_docs, rng), rng)
        b_ids, b_off = ref.csr(ref.sweep_lengths(budget, n_docs, rng), rng)
        dev_src = _upload(a_ids, a_off) + (n_docs,) + _upload(b_ids, b_off) + (n_docs,)
        want = ref.pair_ref(a_ids, a_off, n_docs, b_ids, b_off, n_docs, None, None, n_docs, L, PAD_LEFT | KEEP_TAIL_B, PAD_ID, LONGEST_FIRST, *sg)
        for dt in (0, I64):
            _pair(t, dev_src, None, None, n_docs, L, PAD_LEFT | KEEP_TAIL_B | dt, LONGEST_FIRST, sg, want)
        n_pairs = n_docs + 3                          # one document of B for every pair, A by a random index
        a_idx = [int(x) for x in rng.integers(0, n_docs, size=n_pairs)]
        want = ref.pair_ref(a_ids, a_off, n_docs, b_ids, b_off, n_docs, a_idx, [0] * n_pairs, n_pairs, L, KEEP_TAIL_A, PAD_ID, ONLY_SECOND, *sg)
        _pair(t, dev_src, a_idx, [0] * n_pairs, n_pairs, L, KEEP_TAIL_A | (I64 if L & 1 else 0), ONLY_SECOND, sg, want)
    want = ref.pair_ref(a_ids, a_off, n_docs, b_ids, b_off, n_docs, None, None, 257, L, 0, PAD_ID, ONLY_FIRST, *sg)
    for i, name in enumerate(OUTPUTS):
        _pair(t, dev_src, None, None, 257, L, I64 if i & 1 else 0, ONLY_FIRST, sg, want, null=(name,))
    _pair(t, dev_src, None, None, 257, L, 0, ONLY_FIRST, sg, want, null=OUTPUTS)


def test_pair_two_slices_of_one_csr_and_empty_batch():
    """the two sides as two slices of ONE CSR (off[0] != 0 for B, the same ids pointer); n_pairs == 0 writes nothing; one refusal with a
    real handle"""
    import torch
    from splintr_amd import _ffi
    t = tok(NAME)
    rng = np.random.default_rng(20265)
    n_a, n_b, L = 6, 8, 9
    segs = ((1,), (2,), (3,))
    ids, off = ref.csr([4, 0, 7, 2, 9, 1] + [3, 8, 0, 5, 1, 12, 2, 6], rng)
    d_ids, d_off = _upload(ids, off)
    a_idx, b_idx = [5, 0, 1, 2, 3, 4, 4], [7, 6, 5, 4, 3, 2, 0]
    want = ref.pair_ref(ids, off[:n_a + 1], n_a, ids, off[n_a:], n_b, a_idx, b_idx, 7, L, 0, PAD_ID, LONGEST_FIRST, *segs)
    _pair(t, (d_ids, d_off, n_a, d_ids, d_off[n_a:], n_b), a_idx, b_idx, 7, L, 0, LONGEST_FIRST, segs, want)
    rows, status = Guarded(0, torch.int32), Guarded(1, torch.int32)
    o = _ffi.SplPairOpts(0, L, PAD_ID, 0, *segs)
    args = (t.handle, d_ids.data_ptr(), d_off.data_ptr(), n_a, d_ids.data_ptr(), d_off[n_a:].data_ptr(), n_b, None, None)
    assert _ffi.lib().spl_pair_device(*args, 0, ctypes.byref(o), rows.ptr(), None, None, None, None, None, status.ptr(), _stream()) == 0
    rows.host()
    assert status.host().tolist() == [SENT["int32"]]
    assert _ffi.lib().spl_pair_device(*args, 7, ctypes.byref(o), rows.ptr(), None, None, None, None, None, status.ptr(), _stream()) == -1
    assert "n_pairs exceeds n_a" in _ffi.last_error()


# ------------------------------------------------------------------------------------------ 2. end to end
A_TEXTS = ["What is the capital of France?", "", "how do I reverse a list in python", "Wer hat die Relativitätstheorie entwickelt?", "你好世界",
           "Hello 🌍 World!", "a", "tokenizer seams", "SELECT * FROM users WHERE id = 1;", "The quick brown fox", "   leading spaces",
           "trailing spaces   ", "1234567890", "it's", "naïve café", "def f(x):\n    return x", "question?", "Q", "x" * 40, "end"]
B_TEXTS = ["Paris is the capital and largest city of France.", "an answer to nothing", "", "Albert Einstein, 1905 und 1915.", "世界你好",
           "🌍🌍🌍", "b", "ization of words", "id | name\n1 | root", " jumps over the lazy dog", "more   spaces", "   and more", "0987654321",
           "'s not", "crème brûlée", "print(f(2))", "answer!", "A", "y" * 70, "start"]


def _csr_of(lists):
    off = np.zeros(len(lists) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in lists])
    return np.array([x for l in lists for x in l], dtype=np.uint32), off


def _check_out(out, want, i64=False):
    import torch
    rows, mask, ttype, special, lens, kept, status = out
    assert all(x.device.type == "cuda" for x in out)
    assert rows.dtype == (torch.int64 if i64 else torch.int32) and rows.shape == want[0].shape
    assert mask.dtype == ttype.dtype == special.dtype == torch.uint8 and lens.dtype == kept.dtype == status.dtype == torch.int32
    assert _same_ids(rows.cpu().numpy().reshape(-1), want[0].reshape(-1), i64)
    for got, w in ((mask, want[1]), (ttype, want[2]), (special, want[3]), (lens, want[4]), (kept, want[5])):
        assert got.shape == w.shape and np.array_equal(got.cpu().numpy(), w)
    assert status.cpu().tolist() == [want[6]]


@pytest.mark.parametrize("name", ["cl100k_base", "deepseek_v3"])
def test_encode_batch_pairs_end_to_end(coracle, name):
    """~20 short text pairs: the rows against pair_ref applied to the ORACLE's ids of the two lists encoded separately"""
    import torch
    t = tok(name)
    n = len(A_TEXTS)
    assert len(B_TEXTS) == n
    a_ids, a_off = _csr_of(coracle(name).encode_batch(A_TEXTS))
    b_ids, b_off = _csr_of(coracle(name).encode_batch(B_TEXTS))
    segs = ([1], [2], [2]) if name == "cl100k_base" else ([0], [2, 2], [2])
    for L, kw, flags, trunc in ((16, {}, 0, LONGEST_FIRST),
                                (12, dict(truncation="only_second", padding_side="left", dtype=torch.int64), PAD_LEFT | I64, ONLY_SECOND),
                                (21, dict(truncation="only_first", truncation_side_a="left", truncation_side_b="left"),
                                 KEEP_TAIL_A | KEEP_TAIL_B, ONLY_FIRST)):
        out = t.encode_batch_pairs(A_TEXTS, B_TEXTS, L, pad_id=PAD_ID, prefix=segs[0], middle=segs[1], suffix=segs[2], **kw)
        want = ref.pair_ref(a_ids, a_off, n, b_ids, b_off, n, None, None, n, L, flags, PAD_ID, trunc, *segs)
        _check_out(out, want, bool(flags & I64))
        assert (want[5].sum(axis=1) < np.diff(a_off.astype(np.int64)) + np.diff(b_off.astype(np.int64))).any()      # (something WAS truncated)
    # a_index / b_index name the pairs; one names no text: that side is empty, status says so, check=True raises
    a_index, b_index = [3, 3, 0, 19, 7], [0, 5, 5, 2, 20]
    want = ref.pair_ref(a_ids, a_off, n, b_ids, b_off, n, a_index, b_index, 5, 32, 0, 0, LONGEST_FIRST, *segs)
    assert want[6] == 1
    _check_out(t.encode_batch_pairs(A_TEXTS, B_TEXTS, 32, pad_id=0, a_index=a_index, b_index=b_index, prefix=segs[0], middle=segs[1],
                                    suffix=segs[2]), want)
    with pytest.raises(IndexError, match="names no text"):
        t.encode_batch_pairs(A_TEXTS, B_TEXTS, 32, pad_id=0, a_index=a_index, b_index=b_index, check=True)
    out = t.encode_batch_pairs(A_TEXTS, B_TEXTS, 32, pad_id=0, a_index=a_index[:4], b_index=b_index[:4], check=True)
    assert out[0].shape == (4, 32) and out[6].cpu().tolist() == [0]


def test_encode_batch_pairs_cross_and_special(coracle):
    """cross=True: the 3 x 5 grid, row i * 5 + j = (a_i, b_j); with_special=True: special-token literals in the texts become their ids"""
    t = tok(NAME)
    qs, cs = A_TEXTS[:3], B_TEXTS[3:8]
    a_ids, a_off = _csr_of(coracle(NAME).encode_batch(qs))
    b_ids, b_off = _csr_of(coracle(NAME).encode_batch(cs))
    a_index = [i for i in range(3) for _ in range(5)]
    b_index = [j for _ in range(3) for j in range(5)]
    want = ref.pair_ref(a_ids, a_off, 3, b_ids, b_off, 5, a_index, b_index, 15, 20, 0, 7, LONGEST_FIRST, [1], [2], [3])
    out = t.encode_batch_pairs(qs, cs, 20, pad_id=7, cross=True, prefix=[1], middle=[2], suffix=[3])
    _check_out(out, want)
    assert out[0].shape == (15, 20)
    eot = t._special["<|endoftext|>"]
    sa, sb = ["one<|endoftext|>two", "<|endoftext|>"], ["three <|endoftext|>", "no special here"]
    a_ids, a_off = _csr_of(coracle(NAME).encode_batch(sa, True))
    b_ids, b_off = _csr_of(coracle(NAME).encode_batch(sb, True))
    assert (a_ids == eot).sum() == 2 and (b_ids == eot).sum() == 1
    want = ref.pair_ref(a_ids, a_off, 2, b_ids, b_off, 2, None, None, 2, 16, 0, 0, LONGEST_FIRST, [], [eot], [])
    _check_out(t.encode_batch_pairs(sa, sb, 16, pad_id=0, with_special=True, middle=[eot]), want)
    out = t.encode_batch_pairs([], [], 8, pad_id=0)                       # no pair: empty tensors, nothing launched
    assert out[0].shape == (0, 8) and out[5].shape == (0, 2) and out[6].cpu().tolist() == [0]


def test_pairs_keep_the_seam(coracle):
    """The row's A' and B' are the SEPARATE encodes of the two texts, not the encode of the joined string: where the join changes the
    tokens at the seam the two differ, and the row holds the former."""
    t = tok(NAME)
    a, b = ["Hel", "12", "The quick brown fox"], ["lo, world!", "34", " jumps over the lazy dog"]
    orc = coracle(NAME)
    sep_a, sep_b, joined = orc.encode_batch(a), orc.encode_batch(b), orc.encode_batch([x + y for x, y in zip(a, b)])
    assert [x + y != j for x, y, j in zip(sep_a, sep_b, joined)] == [True, True, False]      # "Hello" and "1234" are tokens of their own; a leading space is a seam already
    rows, mask, ttype, special, lens, kept, status = t.encode_batch_pairs(a, b, 24, pad_id=0)
    rows, kept = rows.cpu().numpy().view(np.uint32), kept.cpu().numpy()
    for p in range(3):
        assert kept[p].tolist() == [len(sep_a[p]), len(sep_b[p])]
        assert rows[p, :kept[p, 0]].tolist() == sep_a[p] and rows[p, kept[p, 0]:kept[p].sum()].tolist() == sep_b[p]
    # pair_device on two batches, and on ONE batch as both sides
    import torch
    from splintr_amd.device import DeviceBatch, encode_device, pair_device
    ba, bb = DeviceBatch(a, _dev()), DeviceBatch(b, _dev())
    encode_device(t, ba)
    encode_device(t, bb)
    a_ids, a_off = _csr_of(sep_a)
    b_ids, b_off = _csr_of(sep_b)
    _check_out(pair_device(t, ba, bb, 10, pad_id=9, middle=[5]), ref.pair_ref(a_ids, a_off, 3, b_ids, b_off, 3, None, None, 3, 10, 0, 9, 0, [], [5], []))
    _check_out(pair_device(t, ba, ba, 10, pad_id=9, b_index=torch.tensor([2, 1, 0], dtype=torch.int32, device=_dev()), dtype=torch.int64),
               ref.pair_ref(a_ids, a_off, 3, a_ids, a_off, 3, None, [2, 1, 0], 3, 10, I64, 9, 0), True)
