"""ctypes wrapper of tests/hostsim/window_sim.cpp (TEST TOOL; builds with g++, no GPU needed)."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "splintr_amd", "csrc")
_LIB = os.path.join(_HERE, "libwindow_sim.so")


def build():
    src = os.path.join(_HERE, "window_sim.cpp")
    deps = [src, os.path.join(_HERE, "gather_sim.h")] + [os.path.join(_CSRC, h) for h in ("spl_k_window.h", "spl_k_collate.h", "spl_common.h")]
    if not os.path.exists(_LIB) or any(os.path.getmtime(d) > os.path.getmtime(_LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", _LIB, src])
    return _LIB


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build())
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        L.ws_geometry.argtypes = [vp]
        L.ws_work_words.restype = u64
        L.ws_work_words.argtypes = [u64]
        L.ws_scan.argtypes = [vp, u64, u32, u32, u32, u64, vp, vp, vp, vp]
        L.ws_gather.argtypes = [vp, vp, vp, u64, u32, u32, u32, u32, u32, u32, vp, u64, vp, vp, vp, vp, vp]
        _lib = L
    return _lib


def geometry():
    g = np.zeros(6, dtype=np.uint32)
    lib().ws_geometry(g.ctypes.data)
    return dict(zip(["lanes", "vec", "span", "window", "scan_span", "totals_chunk"], g.tolist()))


def work_words(n_docs):
    return int(lib().ws_work_words(n_docs))


def scan(off, B, step, rows_cap=0, chunk=None):
    """-> row_off uint64 [n_docs + 1], (need, rows that hold documents), launches: what the scan kernels' arithmetic gives"""
    off = np.ascontiguousarray(off, dtype=np.uint64)
    n_docs = len(off) - 1
    row_off = np.full(n_docs + 2, 0xDEADBEEFDEADBEEF, dtype=np.uint64)
    words = work_words(n_docs)
    work = np.full(words + 1, 0xDEADBEEFDEADBEEF, dtype=np.uint64)
    n = np.zeros(2, dtype=np.uint64)
    launches = np.zeros(1, dtype=np.uint32)
    chunk = geometry()["totals_chunk"] if chunk is None else chunk
    assert lib().ws_scan(off.ctypes.data, n_docs, B, step, chunk, rows_cap, row_off.ctypes.data, n.ctypes.data,
                         work.ctypes.data if words else None, launches.ctypes.data) == 0
    assert row_off[-1] == 0xDEADBEEFDEADBEEF and work[-1] == 0xDEADBEEFDEADBEEF, "written past the end"
    return row_off[:-1], (int(n[0]), int(n[1])), int(launches[0])


def window(ids, off, L, flags, overlap, pad_id, bos_id=0, eos_id=0, rows_cap=None, chunk=None):
    """-> rows uint32 [rows_cap, L], mask uint8, lengths int32 [rows_cap], doc int32, start int64, row_off uint64 [n_docs + 1],
    (need, held), stats: what the scan's and k_window_gather's mapping give"""
    n_docs = len(off) - 1
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    k = (1 if flags & 8 else 0) + (1 if flags & 16 else 0)
    B = L - k
    pre_off, pre_n, _ = scan(off, B, B - overlap, 0, chunk)
    if rows_cap is None:
        rows_cap = pre_n[0]
    row_off, n, launches = scan(off, B, B - overlap, rows_cap, chunk)
    assert np.array_equal(row_off, pre_off) and n[0] == pre_n[0]          # (the scan does not depend on rows_cap)
    total = rows_cap * L
    rows = np.full(total + 1, 0xDEADBEEF, dtype=np.uint32)
    mask = np.full(total + 1, 0x5A, dtype=np.uint8)
    lens = np.full(rows_cap + 1, -7, dtype=np.int32)
    doc = np.full(rows_cap + 1, -7, dtype=np.int32)
    start = np.full(rows_cap + 1, -7, dtype=np.int64)
    stats = np.zeros(4, dtype=np.uint32)
    rc = lib().ws_gather(ids.ctypes.data, off.ctypes.data, row_off.ctypes.data, n_docs, flags, L, pad_id, bos_id, eos_id, overlap,
                         rows.ctypes.data, total, mask.ctypes.data, lens.ctypes.data, doc.ctypes.data, start.ctypes.data, stats.ctypes.data)
    assert rc == 0, "a span held more documents than the window (or the search's bound cut a span short)"
    assert rows[-1] == 0xDEADBEEF and mask[-1] == 0x5A and lens[-1] == -7 and doc[-1] == -7 and start[-1] == -7, "written past the end"
    st = dict(zip(["row_spans", "max_window", "max_rounds", "canary_damage"], stats.tolist()))
    st["launches"] = launches
    return rows[:-1].reshape(rows_cap, L), mask[:-1].reshape(rows_cap, L), lens[:-1], doc[:-1], start[:-1], row_off, n, st
