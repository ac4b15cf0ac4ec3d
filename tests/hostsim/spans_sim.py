"""ctypes wrapper of tests/hostsim/spans_sim.cpp (TEST TOOL; builds with g++, no GPU needed)."""
import ctypes
import os
import subprocess

import numpy as np

from decode_sim import DeviceTable, _aligned

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "splintr_amd", "csrc")
_LIB = os.path.join(_HERE, "libspans_sim.so")
POISON32 = 0xA5A5A5A5
OFF_POISON = 0xA5A5A5A5A5A5A5A5
TAIL = 16                     # canary words behind the span arrays


def build():
    src = os.path.join(_HERE, "spans_sim.cpp")
    deps = [src, os.path.join(_HERE, "gather_sim.h")] + [os.path.join(_CSRC, h) for h in ("spl_k_spans.h", "spl_k_decode_dev.h", "spl_common.h")]
    if not os.path.exists(_LIB) or any(os.path.getmtime(d) > os.path.getmtime(_LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", _LIB, src])
    return _LIB


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build())
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        L.sn_geometry.argtypes = [vp]
        L.sn_entries.argtypes = [vp, vp, u32, vp]
        L.sn_spans.argtypes = [vp, vp, vp, u64, u64, u32, u32, vp, u32, vp, vp, u32, vp, vp, vp, u32, u32, ctypes.c_int] + [vp] * 9
        _lib = L
    return _lib


def geometry():
    g = np.zeros(4, dtype=np.uint32)
    lib().sn_geometry(g.ctypes.data)
    return dict(zip(["lanes", "per_lane", "block", "max_token_bytes"], g.tolist()))


class SpanTable(DeviceTable):
    """decode_sim.DeviceTable plus the characters-per-id table as upload_decode builds it (sn_entry over the same bytes).  `huge`:
    {dense id: length} stretches tok_off so that the id is that long (no byte string of that size exists: spans read no text); its
    entry keeps the characters of its real bytes."""

    def __init__(self, tab, max_id, huge=None):
        super().__init__(tab, max_id)
        n = max_id + 1
        self.nch = np.zeros(n, dtype=np.uint16)
        lib().sn_entries(self.tok_bytes.ctypes.data, self.tok_off.ctypes.data, n, self.nch.ctypes.data)
        self.sp_nch = np.zeros(self.n_sp + 1, dtype=np.uint16)
        lib().sn_entries(self.tok_bytes.ctypes.data, self.sp_off.ctypes.data, self.n_sp, self.sp_nch.ctypes.data)
        if huge:
            lens = np.diff(self.tok_off.astype(np.int64))
            for i, n_bytes in huge.items():
                lens[i] = n_bytes
            off = np.concatenate([[0], np.cumsum(lens)])
            assert off[-1] < (1 << 32)                     # (the side table's lengths are differences of sp_off: they stay)
            self.tok_off = off.astype(np.uint32)


def spans(st, ids, ids_off=None, lengths=None, *, row_len=0, n_cap=None, flags=0, i64=False, lanes=None, mutant=0, want=(1, 1, 1)):
    """What the kernels' mapping gives -> (byte_span [slots, 2] | None, char_span | None, byte_off uint64 [n_docs + 1], char_off | None,
    stats).  want: which of byte_span, char_span, char_off are asked for (the others are passed as null).  Asserts on the way: every
    span entry below `slots` and every offset written exactly ONCE, nothing else written (poisoned destinations, canaries behind them)."""
    ids = _aligned(np.ascontiguousarray(ids, dtype=np.int64 if flags & 1 else np.uint32))
    if row_len:
        n_docs = ids.size // row_len
        off_p, n_cap = None, 0
        ln = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.int32)
        slots = n_docs * row_len
    else:
        ids_off = np.ascontiguousarray(ids_off, dtype=np.uint64)
        n_docs = len(ids_off) - 1
        off_p, ln = ids_off.ctypes.data, None
        n_cap = ids.size if n_cap is None else n_cap
        slots = n_cap
    W = 4 if i64 else 2
    arr = lambda on: (np.full(slots * W + TAIL, POISON32, dtype=np.uint32), np.zeros(slots + TAIL, dtype=np.uint8)) if on else (None, None)
    bs, bs_w = arr(want[0])
    cs, cs_w = arr(want[1])
    boff = np.full(n_docs + 2, OFF_POISON, dtype=np.uint64)
    boff_w = np.zeros(n_docs + 2, dtype=np.uint8)
    coff = np.full(n_docs + 2, OFF_POISON, dtype=np.uint64) if want[2] else None
    coff_w = np.zeros(n_docs + 2, dtype=np.uint8)
    stats = np.zeros(5, dtype=np.uint64)
    p = lambda x: None if x is None else x.ctypes.data
    rc = lib().sn_spans(ids.ctypes.data, off_p, p(ln), n_docs, n_cap, row_len, flags, st.tok_off.ctypes.data, st.max_id, st.sp_ids.ctypes.data,
                        st.sp_off.ctypes.data, st.n_sp, st.sp_bits.ctypes.data, st.nch.ctypes.data, st.sp_nch.ctypes.data, 1 if i64 else 0,
                        lanes or geometry()["lanes"], mutant, p(bs), p(cs), boff.ctypes.data, p(coff), p(bs_w), p(cs_w), boff_w.ctypes.data,
                        coff_w.ctypes.data, stats.ctypes.data)
    assert rc == 0
    s = dict(zip(["canary_damage", "max_rounds", "carries", "carry_reductions", "blocks"], stats.tolist()))
    assert s["canary_damage"] == 0
    assert (boff_w[:-1] == 1).all() and boff_w[-1] == 0 and boff[-1] == OFF_POISON, "a byte offset not written exactly once, or one too many"
    if coff is not None:
        assert (coff_w[:-1] == 1).all() and coff_w[-1] == 0 and coff[-1] == OFF_POISON, "a char offset not written exactly once, or one too many"
    else:
        assert (coff_w == 0).all()
    out = []
    for a, w in ((bs, bs_w), (cs, cs_w)):
        if a is None:
            out.append(None)
            continue
        assert (w[:slots] == 1).all(), "a span entry below `slots` not written exactly once"
        assert (w[slots:] == 0).all() and (a[slots * W:] == POISON32).all(), "written at or beyond `slots`"
        out.append(a[:slots * W].view(np.int64 if i64 else np.int32).reshape(slots, 2).copy())
    return out[0], out[1], boff[:-1].copy(), None if coff is None else coff[:-1].copy(), s
