"""ctypes wrapper of tests/hostsim/mode_sim.cpp (TEST TOOL; builds with g++, no GPU needed)."""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "splintr_amd", "csrc")
_LIB = os.path.join(_HERE, "libmode_sim.so")


def build():
    src = os.path.join(_HERE, "mode_sim.cpp")
    deps = [src, os.path.join(_CSRC, "spl_mode.h")]
    if not os.path.exists(_LIB) or any(os.path.getmtime(d) > os.path.getmtime(_LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", _LIB, src])
    return _LIB


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build())
        L.ms_limits.argtypes = [ctypes.c_void_p]
        L.ms_pick.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint64]
        L.ms_pick.restype = ctypes.c_int
        _lib = L
    return _lib


def limits():
    """(SPL_DIRECT_A_MAX_BYTES, SPL_DIRECT_MAX_BYTES, SPL_QUEUE_MAX_BYTES)"""
    out = (ctypes.c_uint64 * 3)()
    lib().ms_limits(out)
    return tuple(int(v) for v in out)


def pick(force_tile, ext, special, n_bytes):
    """'A' / 'B': tile-owned mode in that geometry, 'Q': queue mode, 'R': refused"""
    return "ABQR"[lib().ms_pick(force_tile, int(ext), int(special), n_bytes)]
