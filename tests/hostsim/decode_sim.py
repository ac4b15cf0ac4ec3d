"""ctypes wrapper of tests/hostsim/decode_sim.cpp (TEST TOOL; builds with g++, no GPU needed)."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "splintr_amd", "csrc")
_LIB = os.path.join(_HERE, "libdecode_sim.so")
POISON = 0xA5
OFF_POISON = 0xA5A5A5A5A5A5A5A5
TAIL = 64


def build():
    src = os.path.join(_HERE, "decode_sim.cpp")
    deps = [src, os.path.join(_HERE, "gather_sim.h"), os.path.join(_CSRC, "spl_k_decode_dev.h"), os.path.join(_CSRC, "spl_common.h")]
    if not os.path.exists(_LIB) or any(os.path.getmtime(d) > os.path.getmtime(_LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", _LIB, src])
    return _LIB


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build())
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        L.ds_geometry.argtypes = [vp]
        L.ds_decode.argtypes = [vp, vp, vp, u64, u64, u32, u32, vp, vp, u32, vp, vp, u32, vp, u32, vp, u64, vp, vp, vp, vp]
        _lib = L
    return _lib


def geometry():
    g = np.zeros(4, dtype=np.uint32)
    lib().ds_geometry(g.ctypes.data)
    return dict(zip(["lanes", "per_lane", "block", "group"], g.tolist()))


class DeviceTable:
    """A decode_ref.Table laid out as upload_decode lays the tables out: a dense offset array over 0 .. max_id (special-only ids fill
    its holes), a sorted side table of the ids beyond it, one bit per dense id that only the special map holds."""

    def __init__(self, tab, max_id):
        off, blob = [0], bytearray()
        bits = np.zeros(max_id // 32 + 1, dtype=np.uint32)
        for i in range(max_id + 1):
            blob += tab.tokens.get(i, b"")
            off.append(len(blob))
            if i in tab.special_only:
                bits[i >> 5] |= np.uint32(1 << (i & 31))
        far = sorted(i for i in tab.tokens if i > max_id)
        assert all(i in tab.special_only for i in far)
        sp_off = []
        for i in far:
            sp_off.append(len(blob))
            blob += tab.tokens[i]
        sp_off.append(len(blob))
        self.max_id = max_id
        self.tok_off = np.array(off, dtype=np.uint32)
        self.tok_bytes = np.frombuffer(bytes(blob) + b"\0" * 16, dtype=np.uint8).copy()
        self.sp_ids = np.array(far + [0], dtype=np.uint32)
        self.sp_off = np.array(sp_off, dtype=np.uint32)
        self.n_sp = len(far)
        self.sp_bits = bits


def _aligned(a, align=64):
    """a copy of a whose data starts at a multiple of `align` bytes (the mapping reads four ids in one piece: 16 or 32 aligned bytes)"""
    raw = np.zeros(a.nbytes + align, dtype=np.uint8)
    at = (-raw.ctypes.data) % align
    out = raw[at:at + a.nbytes].view(a.dtype).reshape(a.shape)
    out[...] = a
    return out


def decode(dt, ids, ids_off=None, lengths=None, *, row_len=0, n_cap=None, flags=0, capacity, lanes=None):
    """What the kernels' mapping gives -> (bytes below min(need, capacity), out_off uint64 [n_docs + 1], stats).  Asserts on the way:
    every byte below min(need, capacity) and every offset written exactly ONCE, nothing else written (poisoned destination, canaries
    behind the capacity and behind the offsets)."""
    ids = _aligned(np.ascontiguousarray(ids, dtype=np.int64 if flags & 1 else np.uint32))
    if row_len:
        n_docs = ids.size // row_len
        off_p, n_cap = None, 0
        ln = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.int32)
    else:
        ids_off = np.ascontiguousarray(ids_off, dtype=np.uint64)
        n_docs = len(ids_off) - 1
        off_p, ln = ids_off.ctypes.data, None
        n_cap = ids.size if n_cap is None else n_cap
    out = np.full(capacity + TAIL, POISON, dtype=np.uint8)
    out_w = np.zeros(capacity + TAIL, dtype=np.uint8)
    out_off = np.full(n_docs + 2, OFF_POISON, dtype=np.uint64)
    off_w = np.zeros(n_docs + 2, dtype=np.uint8)
    stats = np.zeros(6, dtype=np.uint64)
    rc = lib().ds_decode(ids.ctypes.data, off_p, None if ln is None else ln.ctypes.data, n_docs, n_cap, row_len, flags,
                         dt.tok_off.ctypes.data, dt.tok_bytes.ctypes.data, dt.max_id, dt.sp_ids.ctypes.data, dt.sp_off.ctypes.data, dt.n_sp,
                         dt.sp_bits.ctypes.data, lanes or geometry()["lanes"], out.ctypes.data, capacity, out_off.ctypes.data,
                         out_w.ctypes.data, off_w.ctypes.data, stats.ctypes.data)
    assert rc == 0
    st = dict(zip(["wide", "byte", "canary_damage", "max_rounds", "misaligned_wide", "blocks"], stats.tolist()))
    assert (off_w[:-1] == 1).all() and off_w[-1] == 0 and out_off[-1] == OFF_POISON, "an offset not written exactly once, or one too many"
    need = int(out_off[n_docs])
    m = min(need, capacity)
    assert (out_w[:m] == 1).all(), "a byte below min(need, capacity) not written exactly once"
    assert (out_w[m:] == 0).all() and (out[m:] == POISON).all(), "written at or beyond min(need, capacity)"
    assert st["canary_damage"] == 0 and st["misaligned_wide"] == 0
    return out[:m].tobytes(), out_off[:-1].copy(), st
