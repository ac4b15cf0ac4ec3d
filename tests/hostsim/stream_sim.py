"""ctypes wrapper of tests/hostsim/stream_sim.cpp (TEST TOOL; builds with g++, no GPU needed)."""
import ctypes
import os
import subprocess

import numpy as np

from decode_sim import DeviceTable  # noqa: F401  (the tables as upload_decode lays them out)

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "splintr_amd", "csrc")
POISON = 0xA5
WORD_POISON = 0xA5A5A5A5A5A5A5A5
TAIL = 64
MUTANTS = {"": [], "wide_second": ["-DSPL_STREAM_MUTANT_WIDE_SECOND"], "halo2": ["-DSPL_STREAM_HALO=2"]}


def build(mutant=""):
    src = os.path.join(_HERE, "stream_sim.cpp")
    out = os.path.join(_HERE, "libstream_sim%s.so" % ("_" + mutant if mutant else ""))
    deps = [src, os.path.join(_HERE, "seqscan_sim.h")] + [os.path.join(_CSRC, f) for f in ("spl_k_stream.h", "spl_k_seqscan.h", "spl_k_decode_dev.h", "spl_common.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas"] + MUTANTS[mutant] + ["-o", out, src])
    return out


_libs = {}


def lib(mutant=""):
    if mutant not in _libs:
        L = ctypes.CDLL(build(mutant))
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        L.ss_geometry.argtypes = [vp]
        L.ss_step.argtypes = [vp, vp, vp, vp, u64, u32, u32, u32, vp, vp, u32, vp, vp, u32, vp, u32, u32, ctypes.c_int, vp, u64, vp, vp, vp, vp,
                              vp, vp]
        _libs[mutant] = L
    return _libs[mutant]


def geometry(mutant=""):
    g = np.zeros(7, dtype=np.uint32)
    lib(mutant).ss_geometry(g.ctypes.data)
    return dict(zip(["wave", "halo", "seq_block", "one_max", "lanes", "one_lanes", "one_cap"], g.tolist()))


def step(dt, rows, lengths, state_in, *, flags=0, sflags=0, final=None, capacity, lanes=None, chunk=None, three=False, in_place=False,
         mutant=""):
    """One call of the kernels' mapping -> (bytes below min(need, capacity), out_off uint64 [B + 1], state_out uint64 [B]).  Asserts on the
    way: every byte below min(need, capacity), every offset and every state word written exactly ONCE, nothing else written (poisoned
    destinations, canaries behind them).  in_place: state_out IS state_in."""
    rows = np.ascontiguousarray(rows, dtype=np.int64 if flags & 1 else np.uint32)
    B, K = rows.shape
    ln = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.int32)
    fin = None if final is None else np.ascontiguousarray(final, dtype=np.uint8)
    st_in = np.ascontiguousarray(state_in, dtype=np.uint64).copy()
    assert st_in.shape == (B,)
    out = np.full(capacity + TAIL, POISON, dtype=np.uint8)
    out_w = np.zeros(capacity + TAIL, dtype=np.uint8)
    out_off = np.full(B + 2, WORD_POISON, dtype=np.uint64)
    off_w = np.zeros(B + 2, dtype=np.uint8)
    st_out = st_in if in_place else np.full(B + 1, WORD_POISON, dtype=np.uint64)
    st_w = np.zeros(B + 1, dtype=np.uint8)
    stats = np.zeros(2, dtype=np.uint64)
    g = geometry(mutant)
    rc = lib(mutant).ss_step(rows.ctypes.data, None if ln is None else ln.ctypes.data, None if fin is None else fin.ctypes.data,
                             st_in.ctypes.data, B, K, flags, sflags, dt.tok_off.ctypes.data, dt.tok_bytes.ctypes.data, dt.max_id,
                             dt.sp_ids.ctypes.data, dt.sp_off.ctypes.data, dt.n_sp, dt.sp_bits.ctypes.data, lanes or g["wave"],
                             chunk or lanes or g["wave"], int(three), out.ctypes.data, capacity, out_off.ctypes.data, st_out.ctypes.data,
                             out_w.ctypes.data, off_w.ctypes.data, st_w.ctypes.data, stats.ctypes.data)
    assert rc == 0
    assert (off_w[:-1] == 1).all() and off_w[-1] == 0 and out_off[-1] == WORD_POISON, "an offset not written exactly once, or one too many"
    assert (st_w[:B] == 1).all() and st_w[B] == 0, "a state word not written exactly once"
    if not in_place:
        assert st_out[B] == WORD_POISON
    need = int(out_off[B])
    m = min(need, capacity)
    assert (out_w[:m] == 1).all(), "a byte below min(need, capacity) not written exactly once"
    assert (out_w[m:] == 0).all() and (out[m:] == POISON).all(), "written at or beyond min(need, capacity)"
    assert stats[0] == 0, "canary damage"
    return out[:m].tobytes(), out_off[:-1].copy(), st_out[:B].copy()
