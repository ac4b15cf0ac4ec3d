"""ctypes wrapper of tests/hostsim/pair_sim.cpp (TEST TOOL; builds with g++, no GPU needed)."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "splintr_amd", "csrc")
_LIB = os.path.join(_HERE, "libpair_sim.so")


def build():
    src = os.path.join(_HERE, "pair_sim.cpp")
    deps = [src] + [os.path.join(_CSRC, f) for f in ("spl_k_pair.h", "spl_k_collate.h", "spl_common.h")]
    if not os.path.exists(_LIB) or any(os.path.getmtime(d) > os.path.getmtime(_LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", _LIB, src])
    return _LIB


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build())
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        src = [vp, vp, u32, vp, vp, u32, vp, vp, u32, u32, u32, u32, u32, vp, u32, vp, u32, vp, u32]
        L.ps_geometry.argtypes = [vp]
        L.ps_trunc.argtypes = [u64, u64, u32, u32, vp]
        L.ps_trunc.restype = None
        L.ps_grid.argtypes = [u64, vp]
        L.ps_grid.restype = None
        L.ps_span.argtypes = [u32, u32, u32, u32, u32]
        L.ps_span.restype = u64
        L.ps_pair.argtypes = src + [vp] * 7
        L.ps_groups.argtypes = src + [vp, u32] + [vp] * 7
        _lib = L
    return _lib


def geometry():
    g = np.zeros(3, dtype=np.uint32)
    lib().ps_geometry(g.ctypes.data)
    return dict(zip(["lanes", "vec", "span"], g.tolist()))


def trunc(la, lb, budget, mode):
    """the kernel's closed form -> (a', b')"""
    out = np.zeros(2, dtype=np.uint32)
    lib().ps_trunc(la, lb, budget, mode, out.ctypes.data)
    return int(out[0]), int(out[1])


def grid(total):
    out = np.zeros(3, dtype=np.uint32)
    lib().ps_grid(total, out.ctypes.data)
    return tuple(out.tolist())


def span(bx, by, bz, gx, gy):
    return int(lib().ps_span(bx, by, bz, gx, gy))


def _src_args(a_ids, a_off, n_a, b_ids, b_off, n_b, a_idx, b_idx, n_pairs, L, flags, pad_id, trunc_mode, prefix, middle, suffix):
    keep = [np.ascontiguousarray(a_ids, dtype=np.uint32), np.ascontiguousarray(a_off, dtype=np.uint64),
            np.ascontiguousarray(b_ids, dtype=np.uint32), np.ascontiguousarray(b_off, dtype=np.uint64),
            None if a_idx is None else np.ascontiguousarray(a_idx, dtype=np.int32),
            None if b_idx is None else np.ascontiguousarray(b_idx, dtype=np.int32)]
    segs = [np.array(list(s) + [0], dtype=np.uint32) for s in (prefix, middle, suffix)]
    ptr = lambda a: None if a is None else a.ctypes.data
    args = [ptr(keep[0]), ptr(keep[1]), n_a, ptr(keep[2]), ptr(keep[3]), n_b, ptr(keep[4]), ptr(keep[5]), n_pairs, flags, L, pad_id, trunc_mode]
    for s, n in zip(segs, (len(prefix), len(middle), len(suffix))):
        args += [s.ctypes.data, n]
    return args, keep + segs


def pair(a_ids, a_off, n_a, b_ids, b_off, n_b, a_idx, b_idx, n_pairs, L, flags, pad_id, trunc_mode=0, prefix=(), middle=(), suffix=(),
         null=()):
    """-> rows uint32 [n_pairs, L], mask, type, special uint8, lengths int32, kept int32 [n_pairs, 2], status: what k_collate_pair's
    mapping gives.  Every array has one canary element behind it.  null: names of optional outputs passed as NULL (they come back None)."""
    args, keep = _src_args(a_ids, a_off, n_a, b_ids, b_off, n_b, a_idx, b_idx, n_pairs, L, flags, pad_id, trunc_mode, prefix, middle, suffix)
    rows = np.full(n_pairs * L + 1, 0xDEADBEEF, dtype=np.uint32)
    by = {n: np.full(n_pairs * L + 1, 0x5A, dtype=np.uint8) for n in ("mask", "type", "special")}
    lens = np.full(n_pairs + 1, -7, dtype=np.int32)
    kept = np.full(2 * n_pairs + 1, -7, dtype=np.int32)
    status = np.array([0, 0x5A5A5A5A], dtype=np.uint32)
    ptr = lambda name, a: None if name in null else a.ctypes.data
    assert lib().ps_pair(*args, rows.ctypes.data, ptr("mask", by["mask"]), ptr("type", by["type"]), ptr("special", by["special"]),
                         ptr("len", lens), ptr("kept", kept), status.ctypes.data) == 0
    assert rows[-1] == 0xDEADBEEF and all(a[-1] == 0x5A for a in by.values()) and lens[-1] == -7 and kept[-1] == -7 and \
        status[1] == 0x5A5A5A5A, "written past the end"
    for name, a in list(by.items()) + [("len", lens), ("kept", kept)]:
        if name in null:
            assert (a == a[-1]).all(), f"{name} was passed as NULL and written"
    out = lambda name, a: None if name in null else a
    return (rows[:-1].reshape(n_pairs, L), out("mask", by["mask"][:-1].reshape(n_pairs, L)), out("type", by["type"][:-1].reshape(n_pairs, L)),
            out("special", by["special"][:-1].reshape(n_pairs, L)), out("len", lens[:-1]), out("kept", kept[:-1].reshape(n_pairs, 2)),
            int(status[0]))


def groups(a_ids, a_off, n_a, b_ids, b_off, n_b, a_idx, b_idx, n_pairs, L, flags, pad_id, e0, trunc_mode=0, prefix=(), middle=(), suffix=()):
    """The groups of four elements that start at the flat indices e0 (multiples of 4), for outputs that no memory holds:
    -> values uint32 [len(e0), 4], mask / type / special uint8 [len(e0), 4], lengths, kept, status"""
    args, keep = _src_args(a_ids, a_off, n_a, b_ids, b_off, n_b, a_idx, b_idx, n_pairs, L, flags, pad_id, trunc_mode, prefix, middle, suffix)
    e0 = np.ascontiguousarray(e0, dtype=np.uint64)
    g = len(e0)
    v = np.full(4 * g + 1, 0xDEADBEEF, dtype=np.uint32)
    m, ty, sp = (np.full(g + 1, 0x5A5A5A5A, dtype=np.uint32) for _ in range(3))
    lens = np.full(n_pairs + 1, -7, dtype=np.int32)
    kept = np.full(2 * n_pairs + 1, -7, dtype=np.int32)
    status = np.array([0, 0x5A5A5A5A], dtype=np.uint32)
    assert lib().ps_groups(*args, e0.ctypes.data, g, v.ctypes.data, m.ctypes.data, ty.ctypes.data, sp.ctypes.data, lens.ctypes.data,
                           kept.ctypes.data, status.ctypes.data) == 0
    assert v[-1] == 0xDEADBEEF and m[-1] == ty[-1] == sp[-1] == 0x5A5A5A5A and lens[-1] == -7 and kept[-1] == -7 and status[1] == 0x5A5A5A5A
    by = lambda a: a[:-1].copy().view(np.uint8).reshape(g, 4)              # (little endian: byte i is element i)
    return v[:-1].reshape(g, 4), by(m), by(ty), by(sp), lens[:-1], kept[:-1].reshape(n_pairs, 2), int(status[0])
