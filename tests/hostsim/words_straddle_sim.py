"""ctypes wrapper of tests/hostsim/words_straddle_sim.cpp (TEST TOOL; builds with g++, no GPU needed)."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_DATA = os.path.join(_ROOT, "splintr_amd", "data")
_CSRC = os.path.join(_ROOT, "splintr_amd", "csrc")
PATTERNS = {"cl100k": 0, "o200k": 1, "mistral_v3": 2}
TABLES = ("unicode_classes.bin", "unicode_classes_regex.bin")
SWEEPS = ("pairs", "starts", "shapes")
STATS = ["cases", "taken_lead", "taken_cont", "inside", "mismatch", "declined_wrong", "took_wrong", "declined_ts", "declined_edge", "declined_shape"]


def build(broken=0):
    """broken: 0 the header as it is; 5, 6 the form's deliberately wrong variants (SPL_WORDS_SIM_BREAK)"""
    out = os.path.join(_HERE, "libwords_straddle_sim.so" if not broken else f"libwords_straddle_sim_broken{broken}.so")
    src = os.path.join(_HERE, "words_straddle_sim.cpp")
    deps = [src] + [os.path.join(_CSRC, h) for h in ("spl_scan_words.h", "spl_scan_masks.h", "spl_scan.h", "spl_common.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", f"-DSPL_WORDS_SIM_BREAK={broken}", "-o", out, src])
    return out


_libs = {}


def lib(broken=0):
    if broken not in _libs:
        L = ctypes.CDLL(build(broken))
        L.ws_create.restype = ctypes.c_void_p
        L.ws_create.argtypes = [ctypes.c_char_p, ctypes.c_int]
        L.ws_destroy.argtypes = [ctypes.c_void_p]
        for s in SWEEPS:
            getattr(L, "ws_sweep_" + s).argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        _libs[broken] = L
    return _libs[broken]


class WordsStraddleSim:
    def __init__(self, table=TABLES[0], broken=0):
        self._L = lib(broken)
        assert self._L.ws_n_stats() == len(STATS)
        self.n_places, self.n_ascii = self._L.ws_n_places(), self._L.ws_n_ascii()
        with open(os.path.join(_DATA, table), "rb") as f:
            u = f.read()
        self._h = self._L.ws_create(u, len(u))
        if not self._h:
            raise ValueError("bad unicode class table")

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.ws_destroy(self._h)
            self._h = None

    def sweep(self, which, pattern, place):
        """The counts of one sweep (STATS) for one split pattern at one place of the window (PLACES of the source)."""
        st = np.zeros(len(STATS), dtype=np.uint64)
        getattr(self._L, "ws_sweep_" + which)(self._h, PATTERNS[pattern], place, st.ctypes.data)
        return dict(zip(STATS, (int(x) for x in st)))
