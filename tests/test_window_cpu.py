"""spl_window_device without a GPU: the C ABI's refusals, the mapping code the kernels run (splintr_amd/csrc/spl_k_window.h, evaluated for
every output element and every lane of the scan by tests/hostsim/window_sim.cpp) against tests/window_ref.py, window_ref against examples
written out by hand and against the `tokenizers` library's overflowing tokens, and two mutants of the row count."""
import ctypes
import os
import re

import numpy as np
import pytest

import window_ref as ref
from window_ref import BOS, EOS, I64, KEEP_TAIL, PAD_LEFT
from conftest import ROOT

SPL_EINVAL = -1
LS = list(range(1, 10)) + [63, 64, 65]
PAD_ID, BOS_ID, EOS_ID = 0xFFFFFFFF, 0x80000001, 0xFFFFFFFD


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as entry
    entry.build()
    from splintr_amd import _ffi
    return _ffi


@pytest.fixture(scope="module")
def sim():
    import window_sim
    window_sim.lib()
    return window_sim


# ------------------------------------------------------------------------------------------ 1. the C ABI
def test_symbols_and_argument_types(ffi):
    L = ffi.lib()
    assert "spl_window_device" in ffi.SYMBOLS and "spl_window_work_bytes" in ffi.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "splintr_hip.h")).read()
    decl = re.search(r"int spl_window_device\((.*?)\);", hdr, re.S).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert args == ["spl_tokenizer* t", "const uint32_t* d_ids", "const uint64_t* d_out_off", "uint64_t n_docs", "const spl_collate_opts* o",
                    "uint32_t overlap", "void* d_rows", "uint64_t rows_cap", "uint8_t* d_mask", "int32_t* d_len", "int32_t* d_row_doc",
                    "int64_t* d_row_start", "uint64_t* d_row_off", "uint64_t* d_n", "void* d_work", "void* hip_stream"]
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    assert L.spl_window_device.argtypes == [vp, vp, vp, u64, ctypes.POINTER(ffi.SplCollateOpts), ctypes.c_uint32, vp, u64] + [vp] * 8
    assert len(L.spl_window_device.argtypes) == len(args)
    assert "uint64_t spl_window_work_bytes(uint64_t n_docs);" in hdr
    assert L.spl_window_work_bytes.restype is u64 and L.spl_window_work_bytes.argtypes == [u64]
    assert ctypes.sizeof(ffi.SplCollateOpts) == 24            # the struct of pad and pack, unchanged: overlap is an argument


def test_work_bytes_is_a_pure_function_of_n_docs(ffi, sim):
    L = ffi.lib()
    span = sim.geometry()["scan_span"]
    for n in (0, 1, 1000, span - 1, span):
        assert L.spl_window_work_bytes(n) == 0, n           # one span: one launch, no workspace
    for n, spans in ((span + 1, 2), (2 * span, 2), (2 * span + 1, 3), (10000, -(-10000 // span)), ((1 << 31) - 1, -(-((1 << 31) - 1) // span))):
        assert L.spl_window_work_bytes(n) == 8 * (spans + 1) == 8 * sim.work_words(n), n
    assert L.spl_window_work_bytes(10000) == L.spl_window_work_bytes(10000)


def test_refusals_name_their_cause(ffi):
    """Every refusal comes before the handle or the device is touched: a dummy handle (never read) is enough, and none of the addresses
    below is ever dereferenced."""
    L = ffi.lib()
    handle = ctypes.create_string_buffer(64)
    h = ctypes.addressof(handle)
    A = 0x10000                       # an address that is aligned to everything
    O = ffi.SplCollateOpts
    span = 4096

    def win(t=h, ids=A, off=A, n=3, o=None, overlap=0, rows=A, cap=2, mask=A, ln=A, doc=A, start=A, roff=A, dn=A, work=A):
        o = O(0, 8) if o is None else o
        return L.spl_window_device(t, ids, off, n, ctypes.byref(o) if o is not False else None, overlap, rows, cap, mask, ln, doc, start,
                                   roff, dn, work, None)

    def refused(rc, *words):
        msg = L.spl_last_error().decode()
        assert rc == SPL_EINVAL, (rc, msg)
        assert msg.startswith("spl_window_device"), msg
        for w in words:
            assert w in msg, (w, msg)

    # everything collate_check refuses, with its wording
    refused(win(t=None), "null handle")
    refused(win(off=None), "d_out_off")
    refused(win(o=False), "options")
    short = O(0, 8)
    short.struct_size = 0
    refused(win(o=short), "struct_size")
    short.struct_size = 20
    refused(win(o=short), "struct_size")
    refused(win(o=O(0, 0)), "row_len is 0")
    refused(win(o=O(32, 8)), "unknown flag bit 0x20")
    refused(win(o=O(0x80000000 | BOS, 8)), "unknown flag bit 0x80000000")
    refused(win(o=O(BOS | EOS, 1)), "row_len", "BOS + EOS")
    refused(win(n=1 << 31), "n_docs >= 2^31")
    refused(win(rows=A + 8), "d_rows", "16-byte")
    big = (ctypes.c_uint32 * 16)(64, 0, 0, 0, 0, 0, 0xFFFFFFFF, 0xFFFFFFFF)       # a LONGER struct is accepted, its tail ignored
    refused(win(o=ctypes.cast(big, ctypes.POINTER(O)).contents), "row_len is 0")
    assert "struct_size" not in L.spl_last_error().decode()
    # its own
    refused(win(o=O(BOS | EOS, 2)), "row_len", "body budget")                     # row_len == k
    refused(win(o=O(EOS, 1)), "row_len", "body budget")
    refused(win(o=O(0, 8), overlap=8), "overlap")
    refused(win(o=O(BOS | EOS, 8), overlap=6), "overlap")
    refused(win(o=O(BOS, 8), overlap=0xFFFFFFFF), "overlap")
    refused(win(o=O(KEEP_TAIL, 8)), "SPL_COLLATE_KEEP_TAIL")
    refused(win(o=O(KEEP_TAIL | PAD_LEFT | EOS, 8)), "SPL_COLLATE_KEEP_TAIL")
    refused(win(roff=None), "d_row_off is null")
    refused(win(dn=None), "d_n is null")
    refused(win(n=span + 1, work=None), "d_work is null")
    refused(win(mask=A + 2), "d_mask", "4-byte")
    refused(win(ln=A + 4), "d_len", "16-byte")
    refused(win(doc=A + 8), "d_row_doc", "16-byte")
    refused(win(start=A + 8), "d_row_start", "16-byte")
    refused(win(roff=A + 8), "d_row_off", "16-byte")
    refused(win(rows=None), "d_rows is null")
    refused(win(ids=None), "d_ids is null")
    refused(win(cap=1 << 62), "rows_cap * row_len")
    # accepted up to the point where the handle would be read: the flags this call knows, a null workspace for one span
    for fl in (I64, PAD_LEFT, BOS, EOS, I64 | PAD_LEFT | BOS | EOS):
        refused(win(o=O(fl, 8), dn=None), "d_n is null")
    refused(win(n=span, work=None, dn=None), "d_n is null")


# ------------------------------------------------------------------------------------------ 2. the mapping code the kernels run
def _ids32(a):
    return (a & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def _check(sim, ids, off, L, flags, overlap, tag, rows_cap=None, chunk=None, want=None):
    want = want or ref.window_ref(ids, off, L, flags, overlap, PAD_ID, BOS_ID, EOS_ID)
    w_rows, w_mask, w_len, w_doc, w_start, w_off = want
    rows, mask, lens, doc, start, row_off, n, st = sim.window(ids, off, L, flags, overlap, PAD_ID, BOS_ID, EOS_ID, rows_cap=rows_cap, chunk=chunk)
    need = len(w_len)
    cap = rows.shape[0]
    assert np.array_equal(row_off, w_off), tag                      # complete, whatever the cap
    assert n == (need, min(need, cap)), tag
    assert st["canary_damage"] == 0, tag
    m = min(need, cap)
    assert np.array_equal(rows[:m], _ids32(w_rows[:m])) and np.array_equal(mask[:m], w_mask[:m]), tag
    assert np.array_equal(lens[:m], w_len[:m]) and np.array_equal(doc[:m], w_doc[:m]) and np.array_equal(start[:m], w_start[:m]), tag
    assert (rows[m:] == PAD_ID).all() and (mask[m:] == 0).all() and (lens[m:] == 0).all() and (doc[m:] == -1).all() and (start[m:] == 0).all(), tag
    return st


def _flag_sets(L):
    return [f for f in range(32) if not f & KEEP_TAIL and L > ref.n_special(f)]


def test_window_mapping_exhaustive(sim):
    """every L, every flag combination, the overlaps {0, 1, B - 1}, and the document lengths at which the row count changes"""
    rng = np.random.default_rng(20260)
    cases = 0
    for L in LS:
        for flags in _flag_sets(L):
            B = L - ref.n_special(flags)
            for overlap in ref.overlaps(B):
                edges = ref.edge_lengths(B, B - overlap)
                for lens in (edges, [edges[i] for i in rng.integers(0, len(edges), size=int(rng.integers(2, 40)))], [edges[-1]], [0]):
                    ids, off = ref.csr(lens, rng)
                    tag = (L, flags, overlap, lens)
                    _check(sim, ids, off, L, flags, overlap, tag)
                    cases += 1
                ids, off = ref.csr(edges + edges[::-1], rng)
                want = ref.window_ref(ids, off, L, flags, overlap, PAD_ID, BOS_ID, EOS_ID)
                need = len(want[2])
                for cap in (need + 2, need - 1, 0):
                    _check(sim, ids, off, L, flags, overlap, (L, flags, overlap, "cap", cap), rows_cap=cap, want=want)
    assert cases > 1500


def test_window_mapping_no_documents(sim):
    ids, off = ref.csr([])
    for L, flags in ((1, 0), (5, BOS | EOS), (64, PAD_LEFT)):
        for cap in (0, 3):
            st = _check(sim, ids, off, L, flags, 0, (L, flags, cap), rows_cap=cap)
            assert st["row_spans"] == 0 and st["launches"] == 1


def test_window_mapping_one_document_of_thousands_of_windows(sim):
    """one document whose windows fill several spans of the gather: every span's window holds ONE document"""
    rng = np.random.default_rng(3)
    for L, flags, overlap, n_ids in ((3, BOS, 1, 5000), (4, 0, 3, 7000), (9, BOS | EOS | PAD_LEFT, 0, 30000), (65, EOS, 63, 4000)):
        ids, off = ref.csr([2, n_ids, 0, 1], rng)
        st = _check(sim, ids, off, L, flags, overlap, (L, flags, overlap, n_ids))
        assert st["row_spans"] > 3


def test_window_mapping_document_counts_around_the_scan_span(sim):
    """span - 1, span, span + 1 and 2 span + 1 documents: one launch up to the span, three beyond it; with the totals' chunk at 2, three
    spans take two rounds of the second launch.  One-id rows (L = 1) fill every gather span's window with COL_SPAN documents."""
    g = sim.geometry()
    span = g["scan_span"]
    rng = np.random.default_rng(4)
    for n_docs in (span - 1, span, span + 1, 2 * span + 1):
        for L, flags, overlap, top in ((1, 0, 0, 2), (4, BOS, 1, 12), (7, BOS | EOS | PAD_LEFT, 4, 12)):
            lens = rng.integers(0, top, size=n_docs).tolist()
            lens[0] = lens[-1] = 0
            ids, off = ref.csr(lens, rng)
            want = ref.window_ref(ids, off, L, flags, overlap, PAD_ID, BOS_ID, EOS_ID)
            for chunk in (None, 2, 1):
                st = _check(sim, ids, off, L, flags, overlap, (n_docs, L, flags, overlap, chunk), chunk=chunk, want=want)
                assert st["launches"] == (1 if n_docs <= span else 3)
            if L == 1:
                assert st["max_window"] == g["window"] and st["max_rounds"] >= 2


def test_a_gather_span_never_holds_more_documents_than_the_window(sim):
    """Every document has a row, so COL_SPAN elements touch at most COL_SPAN documents: all-empty and one-id documents with the shortest
    rows are the worst case (window_sim returns an error if a span needed more, or if the search's bound cut a span short)."""
    g = sim.geometry()
    rng = np.random.default_rng(5)
    for lens in ([0] * 5000, [1] * 5000, [0, 1] * 2500):
        ids, off = ref.csr(lens, rng)
        for L, flags in ((1, 0), (2, BOS), (2, 0), (3, BOS | EOS)):
            st = _check(sim, ids, off, L, flags, 0, (len(lens), L, flags))
            assert st["max_window"] <= g["window"]


# ------------------------------------------------------------------------------------------ 3. mutants of the row count
def _rows_rule(len_d, B, step):
    return 1 if len_d <= B else 1 + -(-(len_d - B) // step)


def test_case_list_kills_an_off_by_one_in_the_ceiling():
    """Two wrong row counts, and the lengths of edge_lengths() that tell them from the right one:
      floor + 1 instead of the ceiling   1 + (len - B) // step + 1   wrong exactly where len == B + m * step, m >= 1 (one row too
                                          many: an empty window) -- caught by len = B + step, for every step;
      floor instead of the ceiling        1 + (len - B) // step       wrong where len - B is no multiple of step (the tail is lost) --
                                          caught by len = B + 1 and B + step + 1 where step > 1, B + step - 1 where step > 2.
    With step == 1 the floor IS the ceiling: only the first mutant exists there."""
    for L in LS:
        for k in (0, 1, 2):
            B = L - k
            if B < 1:
                continue
            for overlap in ref.overlaps(B):
                step = B - overlap
                edges = ref.edge_lengths(B, step)
                for n in edges:                                   # the rule and the loops of window_ref agree
                    assert len(ref.doc_windows(list(range(n)), B, overlap)) == _rows_rule(n, B, step)
                over = [n for n in edges if n > B and 1 + (n - B) // step + 1 != _rows_rule(n, B, step)]
                assert B + step in over and all((n - B) % step == 0 for n in over), (L, k, overlap)
                under = [n for n in edges if n > B and 1 + (n - B) // step != _rows_rule(n, B, step)]
                if step > 1:
                    assert B + 1 in under and B + step + 1 in under and all((n - B) % step for n in under), (L, k, overlap)
                else:
                    assert not under


# ------------------------------------------------------------------------------------------ 4. window_ref against hand-written examples
def test_ref_by_hand():
    ids = np.array([11, 12, 13, 14, 15, 16, 17, 21], dtype=np.uint32)
    off = np.array([0, 7, 7, 8], dtype=np.uint64)             # documents: [11..17], [], [21]
    rows, mask, lens, doc, start, row_off = ref.window_ref(ids, off, 5, BOS | EOS, 1, 0, 1, 2)     # B = 3, step = 2
    assert rows.tolist() == [[1, 11, 12, 13, 2], [1, 13, 14, 15, 2], [1, 15, 16, 17, 2], [1, 2, 0, 0, 0], [1, 21, 2, 0, 0]]
    assert mask.tolist() == [[1] * 5, [1] * 5, [1] * 5, [1, 1, 0, 0, 0], [1, 1, 1, 0, 0]]
    assert lens.tolist() == [5, 5, 5, 2, 3] and doc.tolist() == [0, 0, 0, 1, 2] and start.tolist() == [0, 2, 4, 0, 0]
    assert row_off.tolist() == [0, 3, 4, 5]
    rows, mask, lens, doc, start, row_off = ref.window_ref(ids, off, 4, PAD_LEFT, 0, 9)            # B = 4, step = 4: the last window is short
    assert rows.tolist() == [[11, 12, 13, 14], [9, 15, 16, 17], [9, 9, 9, 9], [9, 9, 9, 21]]
    assert mask.tolist() == [[1, 1, 1, 1], [0, 1, 1, 1], [0, 0, 0, 0], [0, 0, 0, 1]]
    assert lens.tolist() == [4, 3, 0, 1] and start.tolist() == [0, 4, 0, 0] and row_off.tolist() == [0, 2, 3, 4]
    rows, _, lens, _, start, row_off = ref.window_ref(ids, off, 3, 0, 2, 9)                          # B = 3, step = 1
    assert rows[:5].tolist() == [[11, 12, 13], [12, 13, 14], [13, 14, 15], [14, 15, 16], [15, 16, 17]] and row_off.tolist() == [0, 5, 6, 7]


# ------------------------------------------------------------------------------------------ 5. window_ref against the tokenizers library
def test_ref_against_hugging_face_overflowing_tokens():
    """enable_truncation(max_length = L, stride = overlap): encoding.ids and encoding.overflowing are the windows of one document, BOS and
    EOS through a TemplateProcessing.  (window_ref is the primary reference and never skips; this check runs where the library is.)"""
    tokenizers = pytest.importorskip("tokenizers")
    from tokenizers import Tokenizer, models, pre_tokenizers, processors
    n_vocab = 40
    vocab = {"w%d" % i: i for i in range(n_vocab)}
    vocab.update({"<s>": 100, "</s>": 101, "<unk>": 102})
    rng = np.random.default_rng(6)
    cases = 0
    for flags in (0, BOS, EOS, BOS | EOS):
        k = ref.n_special(flags)
        tok = Tokenizer(models.WordLevel(vocab, unk_token="<unk>"))
        tok.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
        if k:
            tok.post_processor = processors.TemplateProcessing(
                single=("<s> " if flags & BOS else "") + "$A" + (" </s>" if flags & EOS else ""), special_tokens=[("<s>", 100), ("</s>", 101)])
        for L in range(k + 1, 12):
            B = L - k
            for overlap in range(B):
                tok.enable_truncation(max_length=L, stride=overlap)
                for n in list(range(0, 3 * L + 3)) + rng.integers(0, 200, size=3).tolist():
                    doc = rng.integers(0, n_vocab, size=n).tolist()
                    enc = tok.encode(" ".join("w%d" % x for x in doc))
                    got = [enc.ids] + [e.ids for e in enc.overflowing]
                    ids = np.array(doc, dtype=np.uint32)
                    off = np.array([0, n], dtype=np.uint64)
                    rows, _, lens, _, _, _ = ref.window_ref(ids, off, L, flags, overlap, 999, 100, 101)
                    want = [rows[r, :lens[r]].tolist() for r in range(len(lens))]
                    assert got == want, (flags, L, overlap, n)
                    cases += 1
    assert cases > 5000


# ------------------------------------------------------------------------------------------ 6. the Python surface refuses before it works
def test_convenience_method_validates_before_anything_goes_to_the_device():
    """A bad dtype, side string, id, length or overlap raises ValueError BEFORE the texts are packed, uploaded or encoded: a tokenizer
    object without a handle (and texts that could not even be packed) is enough to see it."""
    import torch
    from splintr_amd import Tokenizer
    t = Tokenizer.__new__(Tokenizer)
    unpackable = [b"not a str"]
    with pytest.raises(ValueError, match="dtype"):
        t.encode_batch_windows(unpackable, 8, pad_id=0, dtype=torch.int16)
    with pytest.raises(ValueError, match="padding_side"):
        t.encode_batch_windows(unpackable, 8, pad_id=0, padding_side="up")
    with pytest.raises(ValueError, match="pad_id"):
        t.encode_batch_windows(unpackable, 8, pad_id=1 << 32)
    with pytest.raises(ValueError, match="row length"):
        t.encode_batch_windows(unpackable, 0, pad_id=0)
    with pytest.raises(ValueError, match="room for at least one token"):
        t.encode_batch_windows(unpackable, 2, pad_id=0, bos_id=1, eos_id=2)
    for bad in (8, -1, 7.0, True):
        with pytest.raises(ValueError, match="overlap"):
            t.encode_batch_windows(unpackable, 8, pad_id=0, overlap=bad)
    with pytest.raises(ValueError, match="overlap"):
        t.encode_batch_windows(unpackable, 8, pad_id=0, bos_id=1, eos_id=2, overlap=6)
    assert "stride" in Tokenizer.encode_batch_windows.__doc__
