"""ctypes wrapper of tests/hostsim/collate_sim.cpp (TEST TOOL; builds with g++, no GPU needed)."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "splintr_amd", "csrc")
_LIB = os.path.join(_HERE, "libcollate_sim.so")


def build():
    src = os.path.join(_HERE, "collate_sim.cpp")
    deps = [src, os.path.join(_HERE, "gather_sim.h"), os.path.join(_CSRC, "spl_k_collate.h"), os.path.join(_CSRC, "spl_common.h")]
    if not os.path.exists(_LIB) or any(os.path.getmtime(d) > os.path.getmtime(_LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", _LIB, src])
    return _LIB


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build())
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        L.cs_geometry.argtypes = [vp]
        L.cs_pad.argtypes = [vp, vp, u64, u32, u32, u32, u32, u32, vp, vp, vp]
        L.cs_pack.argtypes = [vp, vp, u64, u32, u32, u32, u32, u32, vp, u64, vp, vp, vp, vp]
        _lib = L
    return _lib


def geometry():
    g = np.zeros(4, dtype=np.uint32)
    lib().cs_geometry(g.ctypes.data)
    return dict(zip(["lanes", "vec", "span", "window"], g.tolist()))


def pad(ids, off, L, flags, pad_id, bos_id=0, eos_id=0):
    """-> rows uint32 [n_docs, L], mask uint8, lengths int32: what k_collate_pad's mapping gives"""
    n_docs = len(off) - 1
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    rows = np.full(n_docs * L + 1, 0xDEADBEEF, dtype=np.uint32)
    mask = np.full(n_docs * L + 1, 0x5A, dtype=np.uint8)
    lens = np.full(n_docs + 1, -7, dtype=np.int32)
    assert lib().cs_pad(ids.ctypes.data, off.ctypes.data, n_docs, flags, L, pad_id, bos_id, eos_id, rows.ctypes.data,
                        mask.ctypes.data, lens.ctypes.data) == 0
    assert rows[-1] == 0xDEADBEEF and mask[-1] == 0x5A and lens[-1] == -7, "written past the end"
    return rows[:-1].reshape(n_docs, L), mask[:-1].reshape(n_docs, L), lens[:-1]


def pack(ids, off, L, flags, pad_id, bos_id=0, eos_id=0, rows_cap=None):
    """-> rows uint32 [rows_cap, L], doc int32, pos int32, (n_rows, S), stats: what k_collate_pack's mapping gives"""
    n_docs = len(off) - 1
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    k = (1 if flags & 8 else 0) + (1 if flags & 16 else 0)
    if rows_cap is None:
        rows_cap = (int(off[-1]) + n_docs * k + L - 1) // L
    total = rows_cap * L
    rows = np.full(total + 1, 0xDEADBEEF, dtype=np.uint32)
    doc = np.full(total + 1, -7, dtype=np.int32)
    pos = np.full(total + 1, -7, dtype=np.int32)
    n = np.zeros(2, dtype=np.uint64)
    stats = np.zeros(4, dtype=np.uint32)
    assert lib().cs_pack(ids.ctypes.data, off.ctypes.data, n_docs, flags, L, pad_id, bos_id, eos_id, rows.ctypes.data, total,
                         doc.ctypes.data, pos.ctypes.data, n.ctypes.data, stats.ctypes.data) == 0
    assert rows[-1] == 0xDEADBEEF and doc[-1] == -7 and pos[-1] == -7, "written past the end"
    st = dict(zip(["window_spans", "global_spans", "max_rounds", "canary_damage"], stats.tolist()))
    return rows[:-1].reshape(rows_cap, L), doc[:-1].reshape(rows_cap, L), pos[:-1].reshape(rows_cap, L), (int(n[0]), int(n[1])), st
