"""ctypes wrapper of tests/hostsim/maskapply_sim.cpp (TEST TOOL; builds with g++, no GPU needed)."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "splintr_amd", "csrc")
F32, F16, BF16 = 0, 1, 2
ELEM = {F32: 4, F16: 2, BF16: 2}
NINF = {F32: 0xFF800000, F16: 0xFC00, BF16: 0xFF80}
UINT = {F32: np.uint32, F16: np.uint16, BF16: np.uint16}


def build():
    src = os.path.join(_HERE, "maskapply_sim.cpp")
    out = os.path.join(_HERE, "libmaskapply_sim.so")
    deps = [src] + [os.path.join(_CSRC, f) for f in ("spl_k_maskapply.h", "spl_common.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", out, src])
    return out


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build())
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        L.ma_sim_piece.argtypes = [u64, u32, u32, u64, vp]
        L.ma_sim_grid_pieces.restype = u64
        L.ma_sim_grid_pieces.argtypes = [u32, u32]
        L.ma_sim.argtypes = [vp, u64, u64, u32, u64, u32, u64, vp, u32, u64, u64, vp, vp, vp, vp, vp]
        _lib = L
    return _lib


def piece(A, es, n_eff, p):
    """ma_piece and ma_n_pieces -> dict(addr, c0, j0, n, n_pieces)"""
    out = np.zeros(5, dtype=np.uint64)
    lib().ma_sim_piece(A, es, n_eff, p, out.ctypes.data)
    return dict(zip(["addr", "c0", "j0", "n", "n_pieces"], (int(x) for x in out)))


def forced(shape, mask, live, n_cols):
    """bool [R, stride]: the elements that must become -inf"""
    R = shape[0]
    sel = np.zeros(shape, dtype=bool)
    n_eff = min(n_cols, 32 * mask.shape[1])
    if R and n_eff:
        bits = np.unpackbits(np.ascontiguousarray(mask).view(np.uint8).reshape(R, -1), axis=1, bitorder="little")[:, :n_eff].astype(bool)
        rows = np.ones(R, dtype=bool) if live is None else np.asarray(live).astype(bool)
        sel[:, :n_eff] = ~bits & rows[:, None]
    return sel


def expected(vals, dtype, mask, live, n_cols):
    """numpy on the bit patterns: vals uint [R, stride] -> what the call must leave"""
    want = vals.copy()
    want[forced(vals.shape, mask, live, n_cols)] = NINF[dtype]
    return want


def run(vals, dtype, mask, *, n_cols, base_elems=0, live=None, mask_stride=None, tail_elems=24):
    """k_mask_apply's code over a guarded buffer.  vals uint16 / uint32 [R, row_stride]: the bit patterns of the rows with their padding;
    the first row begins base_elems elements behind a 16-byte boundary; mask uint32 [R, n_words].  Returns (vals after, kinds): the lanes
    that did nothing, a 16-byte store, load and store, element stores.  Asserts on the way: no access outside the buffer, no byte stored
    twice, every byte stored is one whose value had to change or a byte of a piece that was loaded first, nothing in front of the first
    row, behind the last or in a row's padding written, the mask rows of rows that are not live not read."""
    es = ELEM[dtype]
    vals = np.ascontiguousarray(vals, dtype=UINT[dtype])
    R, stride = vals.shape
    n_words = mask.shape[1]
    raw = np.zeros(16 + (base_elems + R * stride + tail_elems) * es + 32, dtype=np.uint8)
    pad = (-raw.ctypes.data) % 16
    buf = raw[pad:pad + ((base_elems + R * stride + tail_elems) * es + 15) // 16 * 16]
    assert buf.ctypes.data % 16 == 0
    buf[:] = 0xC7
    body = buf[base_elems * es:(base_elems + R * stride) * es].view(UINT[dtype]).reshape(R, stride)
    body[:] = vals
    before = buf.copy()
    ms = n_words if mask_stride is None else mask_stride
    m = np.full((R, ms), 0xA5A5A5A5, dtype=np.uint32)
    m[:, :n_words] = mask
    st, ld = np.zeros(len(buf), dtype=np.uint8), np.zeros(len(buf), dtype=np.uint8)
    mask_r = np.zeros(m.size + 1, dtype=np.uint8)
    stats = np.zeros(5, dtype=np.uint64)
    lv = None if live is None else np.ascontiguousarray(live, dtype=np.uint8)
    rc = lib().ma_sim(buf.ctypes.data, len(buf), base_elems * es, dtype, R, n_cols, stride, m.ctypes.data, n_words, ms, m.size,
                      None if lv is None else lv.ctypes.data, st.ctypes.data, ld.ctypes.data, mask_r.ctypes.data, stats.ctypes.data)
    assert rc == 0, rc
    assert stats[0] == 0, "an access outside the buffer, or a misaligned one"
    assert st.max(initial=0) <= 1, "a byte stored twice"
    changed_ok = np.zeros(len(buf), dtype=bool)
    changed_ok[base_elems * es:(base_elems + R * stride) * es] = np.repeat(forced(vals.shape, mask, live, n_cols).reshape(-1), es)
    # a stored byte either had to become -inf, or belongs to a whole piece that was loaded first (and then keeps its value)
    assert ((st == 0) | changed_ok | (ld == 1)).all(), "a store without a load to a byte that must keep its value"
    outside = np.ones(len(buf), dtype=bool)
    for r in range(R):
        a = (base_elems + r * stride) * es
        outside[a:a + n_cols * es] = False
    assert (st[outside] == 0).all(), "written in front of a row, behind it, or in its padding"
    assert (buf[outside] == before[outside]).all()
    mr = mask_r[:m.size].reshape(R, ms)
    assert (mr[:, n_words:] == 0).all(), "the mask's padding was read"
    if live is not None:
        assert (mr[~np.asarray(live).astype(bool)] == 0).all(), "the mask row of a row that is not live was read"
    got = buf[base_elems * es:(base_elems + R * stride) * es].view(UINT[dtype]).reshape(R, stride).copy()
    return got, [int(x) for x in stats[1:5]]
