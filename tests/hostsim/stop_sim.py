"""ctypes wrapper of tests/hostsim/stop_sim.cpp (TEST TOOL; builds with g++, no GPU needed)."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "splintr_amd", "csrc")
POISON = 0xA5
WORD_POISON = 0xA5A5A5A5A5A5A5A5
HIT_POISON = -0x5A5A5A5B
TAIL = 64
WORDS = 10
MUTANTS = {"": [], "halo62": ["-DSPL_STOP_HALO=62"], "shortest": ["-DSPL_STOP_MUTANT_SHORTEST"]}


def build(mutant=""):
    src = os.path.join(_HERE, "stop_sim.cpp")
    out = os.path.join(_HERE, "libstop_sim%s.so" % ("_" + mutant if mutant else ""))
    deps = [src, os.path.join(_HERE, "seqscan_sim.h")] + [os.path.join(_CSRC, f) for f in ("spl_k_stop.h", "spl_k_seqscan.h", "spl_common.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas"] + MUTANTS[mutant] + ["-o", out, src])
    return out


_libs = {}


def lib(mutant=""):
    if mutant not in _libs:
        L = ctypes.CDLL(build(mutant))
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        L.sp_geometry.argtypes = [vp]
        L.sp_step.argtypes = [vp, u64, vp, u64, vp, vp, vp, u32, vp, u32, u32, ctypes.c_int, vp, u64, vp, vp, vp, vp, vp, vp, vp, vp]
        _libs[mutant] = L
    return _libs[mutant]


def geometry(mutant=""):
    g = np.zeros(8, dtype=np.uint32)
    lib(mutant).sp_geometry(g.ctypes.data)
    return dict(zip(["wave", "halo", "seq_block", "one_max", "lanes", "one_lanes", "one_cap", "table_bytes"], g.tolist()))


def step(in_bytes, in_off, state_in, table, *, mask=None, final=None, flags=0, capacity, in_capacity=None, lanes=None, chunk=None, three=False,
         in_place=False, mutant=""):
    """One call of the kernels' mapping -> (bytes below min(need, capacity), out_off uint64 [B + 1], hit int32 [B], state_out uint64 [B, 10]).
    Asserts on the way: every byte below min(need, capacity), every offset, every hit and every state word written exactly ONCE, nothing
    else written (poisoned destinations, canaries behind them).  in_place: state_out IS state_in."""
    src = np.frombuffer(bytes(in_bytes), dtype=np.uint8).copy() if not isinstance(in_bytes, np.ndarray) else np.ascontiguousarray(in_bytes, dtype=np.uint8)
    off = np.ascontiguousarray(in_off, dtype=np.uint64)
    B = off.shape[0] - 1
    st_in = np.ascontiguousarray(state_in, dtype=np.uint64).copy()
    assert st_in.shape == (B, WORDS)
    tab = np.ascontiguousarray(table, dtype=np.uint8)
    g = geometry(mutant)
    assert tab.shape == (g["table_bytes"],)
    msk = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint64)
    fin = None if final is None else np.ascontiguousarray(final, dtype=np.uint8)
    in_cap = src.shape[0] if in_capacity is None else in_capacity
    out = np.full(capacity + TAIL, POISON, dtype=np.uint8)
    out_w = np.zeros(capacity + TAIL, dtype=np.uint8)
    out_off = np.full(B + 2, WORD_POISON, dtype=np.uint64)
    off_w = np.zeros(B + 2, dtype=np.uint8)
    st_out = st_in if in_place else np.full((B + 1, WORDS), WORD_POISON, dtype=np.uint64)
    st_w = np.zeros((B + 1, WORDS), dtype=np.uint8)
    hit = np.full(B + 1, HIT_POISON, dtype=np.int32)
    hit_w = np.zeros(B + 1, dtype=np.uint8)
    stats = np.zeros(2, dtype=np.uint64)
    ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data
    rc = lib(mutant).sp_step(ptr(src), in_cap, off.ctypes.data, B, tab.ctypes.data, ptr(msk), ptr(fin), flags, st_in.ctypes.data,
                             lanes or g["wave"], chunk or lanes or g["wave"], int(three), out.ctypes.data, capacity, out_off.ctypes.data,
                             st_out.ctypes.data, hit.ctypes.data, out_w.ctypes.data, off_w.ctypes.data, st_w.ctypes.data, hit_w.ctypes.data,
                             stats.ctypes.data)
    assert rc == 0
    assert (off_w[:-1] == 1).all() and off_w[-1] == 0 and out_off[-1] == WORD_POISON, "an offset not written exactly once, or one too many"
    assert (st_w[:B] == 1).all() and (st_w[B] == 0).all(), "a state word not written exactly once"
    assert (hit_w[:B] == 1).all() and hit_w[B] == 0 and hit[B] == HIT_POISON, "a hit not written exactly once"
    if not in_place:
        assert (st_out[B] == WORD_POISON).all()
    need = int(out_off[B])
    m = min(need, capacity)
    assert (out_w[:m] == 1).all(), "a byte below min(need, capacity) not written exactly once"
    assert (out_w[m:] == 0).all() and (out[m:] == POISON).all(), "written at or beyond min(need, capacity)"
    assert stats[0] == 0, "canary damage"
    return out[:m].tobytes(), out_off[:-1].copy(), hit[:B].copy(), st_out[:B].copy()
