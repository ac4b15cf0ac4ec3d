"""spl_pad_device / spl_pack_device without a GPU: the C ABI's refusals, the mapping code the kernels run (splintr_amd/csrc/spl_k_collate.h,
evaluated for every output element by tests/hostsim/collate_sim.cpp) against tests/collate_ref.py, and collate_ref against examples
written out by hand."""
import ctypes
import os
import re

import numpy as np
import pytest

import collate_ref as ref
from collate_ref import BOS, EOS, I64, KEEP_TAIL, PAD_LEFT
from conftest import ROOT

SPL_EINVAL = -1
LS = list(range(1, 10)) + [63, 64, 65]


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as entry
    entry.build()
    from splintr_amd import _ffi
    return _ffi


@pytest.fixture(scope="module")
def sim():
    import collate_sim
    collate_sim.lib()
    return collate_sim


# ------------------------------------------------------------------------------------------ 1. the C ABI
def test_symbols_and_struct_layout(ffi):
    L = ffi.lib()
    assert hasattr(L, "spl_pad_device") and hasattr(L, "spl_pack_device")
    hdr = open(os.path.join(ROOT, "include", "splintr_hip.h")).read()
    body = re.search(r"typedef struct spl_collate_opts \{(.*?)\} spl_collate_opts;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip() for decl in re.findall(r"uint32_t ([^;]+);", body) for n in decl.split(",")]
    assert fields == ["struct_size", "flags", "row_len", "pad_id", "bos_id", "eos_id"]
    O = ffi.SplCollateOpts
    assert [f[0] for f in O._fields_] == fields and all(f[1] is ctypes.c_uint32 for f in O._fields_)
    assert ctypes.sizeof(O) == 24 and [getattr(O, f).offset for f in fields] == [0, 4, 8, 12, 16, 20]
    assert O(3, 5).struct_size == 24
    for name, val in (("I64", 1), ("PAD_LEFT", 2), ("KEEP_TAIL", 4), ("BOS", 8), ("EOS", 16)):
        assert re.search(r"#define SPL_COLLATE_%s\s+%du\b" % (name, val), hdr), name
        assert getattr(ffi, "SPL_COLLATE_" + name) == val


def test_refusals_name_their_cause(ffi):
    """Every refusal comes before the handle or the device is touched: a dummy handle (never read) is enough, and none of the addresses
    below is ever dereferenced."""
    L = ffi.lib()
    handle = ctypes.create_string_buffer(64)
    h = ctypes.addressof(handle)
    A = 0x10000                       # an address that is aligned to everything
    O = ffi.SplCollateOpts

    def pad(t=h, ids=A, off=A, n=3, o=None, rows=A, mask=A, ln=A):
        o = O(0, 8) if o is None else o
        return L.spl_pad_device(t, ids, off, n, ctypes.byref(o) if o is not False else None, rows, mask, ln, None)

    def pack(t=h, ids=A, off=A, n=3, o=None, rows=A, cap=2, doc=A, pos=A, dn=A):
        o = O(0, 8) if o is None else o
        return L.spl_pack_device(t, ids, off, n, ctypes.byref(o) if o is not False else None, rows, cap, doc, pos, dn, None)

    def refused(rc, *words):
        msg = L.spl_last_error().decode()
        assert rc == SPL_EINVAL, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    for call, name in ((pad, "spl_pad_device"), (pack, "spl_pack_device")):
        refused(call(t=None), name, "null handle")
        refused(call(off=None), name, "d_out_off")
        refused(call(o=False), name, "options")
        refused(call(rows=None), name, "d_rows is null")
        refused(call(ids=None), name, "d_ids is null")
        short = O(0, 8)
        short.struct_size = 0
        refused(call(o=short), name, "struct_size")
        short.struct_size = 20
        refused(call(o=short), name, "struct_size")
        refused(call(o=O(0, 0)), name, "row_len is 0")
        refused(call(o=O(32, 8)), name, "unknown flag bit 0x20")
        refused(call(o=O(0x80000000 | BOS, 8)), name, "unknown flag bit 0x80000000")
        refused(call(rows=A + 8), name, "d_rows", "16-byte")
        refused(call(n=1 << 31), name, "n_docs >= 2^31")
        # a LONGER struct is accepted and its tail ignored: the refusal that follows is about something else
        big = (ctypes.c_uint32 * 16)(64, 0, 0, 0, 0, 0, 0xFFFFFFFF, 0xFFFFFFFF)
        rc = call(o=ctypes.cast(big, ctypes.POINTER(O)).contents)
        refused(rc, name, "row_len is 0")
        assert "struct_size" not in L.spl_last_error().decode()
    refused(pad(o=O(BOS | EOS, 1)), "row_len", "BOS + EOS")
    refused(pad(mask=A + 2), "d_mask", "4-byte")
    refused(pad(ln=A + 4), "d_len", "16-byte")
    refused(pack(o=O(PAD_LEFT, 8)), "pad-mode")
    refused(pack(o=O(KEEP_TAIL | EOS, 8)), "pad-mode")
    refused(pack(doc=A + 4), "d_doc", "16-byte")
    refused(pack(pos=A + 8), "d_pos", "16-byte")
    refused(pack(dn=None), "d_n is null")
    refused(pack(cap=1 << 62), "rows_cap * row_len")
    # pad with nothing to do is not an error, and needs neither rows nor ids
    assert pad(n=0, rows=None, ids=None, mask=None, ln=None) == 0


# ------------------------------------------------------------------------------------------ 2. the mapping code the kernels run
def _ids32(a):
    return (a & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def _check_pad(sim, ids, off, L, flags, tag):
    want = ref.pad_ref(ids, off, L, flags, 0xFFFFFFFF, 0x80000001, 0xFFFFFFFD)
    got = sim.pad(ids, off, L, flags, 0xFFFFFFFF, 0x80000001, 0xFFFFFFFD)
    assert np.array_equal(got[0], _ids32(want[0])), tag
    assert np.array_equal(got[1], want[1]), tag
    assert np.array_equal(got[2], want[2]), tag


def _check_pack(sim, ids, off, L, flags, tag, rows_cap=None):
    w_rows, w_doc, w_pos, n_rows, S = ref.pack_ref(ids, off, L, flags, 0xFFFFFFFF, 0x80000001, 0xFFFFFFFD)
    rows, doc, pos, n, st = sim.pack(ids, off, L, flags, 0xFFFFFFFF, 0x80000001, 0xFFFFFFFD, rows_cap=rows_cap)
    assert n == (n_rows, S), tag
    assert st["canary_damage"] == 0, tag
    m = min(n_rows, rows.shape[0])
    assert np.array_equal(rows[:m], _ids32(w_rows[:m])), tag
    assert np.array_equal(doc[:m], w_doc[:m]), tag
    assert np.array_equal(pos[:m], w_pos[:m]), tag
    assert (rows[m:] == 0xFFFFFFFF).all() and (doc[m:] == -1).all() and (pos[m:] == 0).all(), tag     # rows the stream does not reach
    return st


def test_pad_mapping_exhaustive(sim):
    rng = np.random.default_rng(20250)
    cases = 0
    for L in LS:
        for flags in range(32):
            k = ref.n_special(flags)
            if L < k:                          # refused by the C ABI (row_len < BOS + EOS): no mapping to check
                continue
            for n_docs in (1, int(rng.integers(2, 40)), 40):
                ids, off = ref.csr(ref.sweep_lengths(L, k, n_docs, rng), rng)
                _check_pad(sim, ids, off, L, flags, (L, flags, n_docs, off.tolist()))
                cases += 1
    assert cases > 1000


def test_pack_mapping_exhaustive(sim):
    rng = np.random.default_rng(20251)
    for L in LS:
        for flags in (0, I64, BOS, EOS, BOS | EOS, I64 | BOS, I64 | EOS, I64 | BOS | EOS):
            k = ref.n_special(flags)
            for n_docs in (1, int(rng.integers(2, 40)), 40):
                ids, off = ref.csr(ref.sweep_lengths(L, k, n_docs, rng), rng)
                tag = (L, flags, n_docs, off.tolist())
                _check_pack(sim, ids, off, L, flags, tag)
                n_rows = (int(off[-1]) + n_docs * k + L - 1) // L
                _check_pack(sim, ids, off, L, flags, tag + ("cap+2",), rows_cap=n_rows + 2)
                if n_rows:
                    _check_pack(sim, ids, off, L, flags, tag + ("cap-1",), rows_cap=n_rows - 1)


def _runs(n_empty):
    """document-length lists with runs of empty documents: between two documents, at the start, at the end, everywhere"""
    return {
        "between": [5] + [0] * n_empty + [7],
        "start": [0] * n_empty + [3, 0, 4],
        "end": [6, 2] + [0] * n_empty,
        "both": [0] * n_empty + [9] + [0] * n_empty + [1] + [0] * n_empty,
        "all_empty": [0] * n_empty,
        "ones_and_runs": ([1] * 700 + [0] * n_empty) * 2 + [1] * 700,
    }


@pytest.mark.parametrize("n_empty", [3, 1000, 5000])
def test_pack_mapping_empty_runs(sim, n_empty):
    """With k = 0 empty documents share their start with their successor: the LARGEST document with start <= p is the one that owns p.
    5000 of them put more starts into one workgroup's span than the window holds: such spans search the global array."""
    g = sim.geometry()
    rng = np.random.default_rng(7)
    for name, lens in _runs(n_empty).items():
        ids, off = ref.csr(lens, rng)
        for L in (1, 3, 64, 65):
            for flags in (0, BOS, EOS, BOS | EOS):
                st = _check_pack(sim, ids, off, L, flags, (name, n_empty, L, flags))
                k = ref.n_special(flags)
                S = int(off[-1]) + len(lens) * k
                if k:
                    assert st["global_spans"] == 0          # every document takes a position: a span never holds more than the window
                elif n_empty > g["window"] and name in ("between", "both", "ones_and_runs"):
                    assert st["global_spans"] > 0, (name, L)       # (a run at the very start or end lies outside every span's bounds)
                elif n_empty + 3 <= g["window"] and name in ("between", "start", "end", "all_empty"):
                    assert st["global_spans"] == 0 and (st["window_spans"] > 0) == (S > 0)


def test_pack_mapping_many_documents(sim):
    """5 000 and 70 000 one-token documents: the cooperative search needs more than one round, and every span's window is full or nearly."""
    rng = np.random.default_rng(11)
    for n_docs, rounds in ((5000, 2), (70000, 3)):
        ids, off = ref.csr([1] * n_docs, rng)
        for flags, L in ((0, 7), (BOS, 64), (BOS | EOS, 5)):
            st = _check_pack(sim, ids, off, L, flags, (n_docs, flags, L))
            assert st["max_rounds"] == rounds and st["global_spans"] == 0


def test_pad_mapping_many_rows(sim):
    """rows that straddle lanes and workgroups: more than one span, L no multiple of the lane's group"""
    rng = np.random.default_rng(12)
    for n_docs, L in ((257, 5), (1025, 3), (300, 65)):
        for flags in (0, PAD_LEFT | KEEP_TAIL | BOS, EOS | KEEP_TAIL, BOS | EOS | PAD_LEFT):
            k = ref.n_special(flags)
            ids, off = ref.csr(ref.sweep_lengths(L, k, n_docs, rng), rng)
            _check_pad(sim, ids, off, L, flags, (n_docs, L, flags))


# ------------------------------------------------------------------------------------------ 3. collate_ref against hand-written examples
def test_ref_pad_by_hand():
    ids = np.array([11, 12, 13, 14, 15, 21], dtype=np.uint32)
    off = np.array([0, 5, 5, 6], dtype=np.uint64)             # documents: [11..15], [], [21]
    rows, mask, lens = ref.pad_ref(ids, off, 4, BOS | EOS, 0, 1, 2)
    assert rows.tolist() == [[1, 11, 12, 2], [1, 2, 0, 0], [1, 21, 2, 0]]
    assert mask.tolist() == [[1, 1, 1, 1], [1, 1, 0, 0], [1, 1, 1, 0]] and lens.tolist() == [4, 2, 3]
    rows, mask, lens = ref.pad_ref(ids, off, 4, BOS | EOS | KEEP_TAIL | PAD_LEFT, 0, 1, 2)
    assert rows.tolist() == [[1, 14, 15, 2], [0, 0, 1, 2], [0, 1, 21, 2]]
    assert mask.tolist() == [[1, 1, 1, 1], [0, 0, 1, 1], [0, 1, 1, 1]] and lens.tolist() == [4, 2, 3]
    rows, mask, lens = ref.pad_ref(ids, off, 3, 0, 9)
    assert rows.tolist() == [[11, 12, 13], [9, 9, 9], [21, 9, 9]] and lens.tolist() == [3, 0, 1]


def test_ref_pack_document_across_two_row_boundaries():
    # one document of 8 ids behind a document of 2, rows of 3, EOS on: the stream is 10 20 E 1 2 3 4 5 6 7 8 E
    ids = np.array([10, 20, 1, 2, 3, 4, 5, 6, 7, 8], dtype=np.uint32)
    off = np.array([0, 2, 10], dtype=np.uint64)
    rows, doc, pos, n_rows, S = ref.pack_ref(ids, off, 3, EOS, 0, eos_id=99)
    assert (n_rows, S) == (4, 12)
    assert rows.tolist() == [[10, 20, 99], [1, 2, 3], [4, 5, 6], [7, 8, 99]]
    assert doc.tolist() == [[0, 0, 0], [1, 1, 1], [1, 1, 1], [1, 1, 1]]
    assert pos.tolist() == [[0, 1, 2], [0, 1, 2], [0, 1, 2], [0, 1, 2]]       # the position restarts with every row
    # rows of 4: the second document starts in the middle of row 0 and crosses the boundaries at 4 and 8
    rows, doc, pos, n_rows, S = ref.pack_ref(ids, off, 4, EOS, 0, eos_id=99)
    assert rows.tolist() == [[10, 20, 99, 1], [2, 3, 4, 5], [6, 7, 8, 99]]
    assert doc.tolist() == [[0, 0, 0, 1], [1, 1, 1, 1], [1, 1, 1, 1]]
    assert pos.tolist() == [[0, 1, 2, 0], [0, 1, 2, 3], [0, 1, 2, 3]]


def test_ref_pack_empty_documents_and_tail_by_hand():
    ids = np.array([5, 6, 7], dtype=np.uint32)
    off = np.array([0, 0, 2, 2, 2, 3, 3], dtype=np.uint64)    # [], [5 6], [], [], [7], []
    rows, doc, pos, n_rows, S = ref.pack_ref(ids, off, 2, 0, 8)           # k = 0: empty documents leave no trace
    assert (n_rows, S) == (2, 3)
    assert rows.tolist() == [[5, 6], [7, 8]] and doc.tolist() == [[1, 1], [4, -1]] and pos.tolist() == [[0, 1], [0, 0]]
    rows, doc, pos, n_rows, S = ref.pack_ref(ids, off, 4, BOS, 8, bos_id=1)     # k = 1: every document shows its BOS
    assert (n_rows, S) == (3, 9)
    assert rows.tolist() == [[1, 1, 5, 6], [1, 1, 1, 7], [1, 8, 8, 8]]
    assert doc.tolist() == [[0, 1, 1, 1], [2, 3, 4, 4], [5, -1, -1, -1]]
    assert pos.tolist() == [[0, 0, 1, 2], [0, 0, 0, 1], [0, 0, 0, 0]]


# ------------------------------------------------------------------------------------------ 4. the Python surface refuses before it works
def test_convenience_methods_validate_before_anything_goes_to_the_device():
    """A bad dtype, side string, id or length raises ValueError BEFORE the texts are packed, uploaded or encoded: a tokenizer object
    without a handle (and texts that could not even be packed) is enough to see it."""
    import torch
    from splintr_amd import Tokenizer
    t = Tokenizer.__new__(Tokenizer)
    unpackable = [b"not a str"]
    with pytest.raises(ValueError, match="dtype"):
        t.encode_batch_padded(unpackable, 8, pad_id=0, dtype=torch.int16)
    with pytest.raises(ValueError, match="dtype"):
        t.encode_batch_packed(unpackable, 8, pad_id=0, dtype=torch.float32)
    with pytest.raises(ValueError, match="padding_side"):
        t.encode_batch_padded(unpackable, 8, pad_id=0, padding_side="up")
    with pytest.raises(ValueError, match="truncation_side"):
        t.encode_batch_padded(unpackable, 8, pad_id=0, truncation_side="middle")
    with pytest.raises(ValueError, match="pad_id"):
        t.encode_batch_packed(unpackable, 8, pad_id=1 << 32)
    with pytest.raises(ValueError, match="row length"):
        t.encode_batch_padded(unpackable, 0, pad_id=0)
