"""ctypes wrapper of tests/hostsim/words_sim.cpp (TEST TOOL; builds with g++, no GPU needed)."""
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
SWEEPS = ("positions", "fillings", "guards")


def build(broken=0):
    """broken: 0 the header as it is; 1, 2 its deliberately wrong variants (SPL_WORDS_SIM_BREAK); "full": without the sub-case of one
    character (-DSPL_WORD_TWO_ONE=0: every word through the form for up to three characters)"""
    out = os.path.join(_HERE, "libwords_sim.so" if not broken else f"libwords_sim_{'broken' if broken != 'full' else ''}{broken}.so")
    src = os.path.join(_HERE, "words_sim.cpp")
    deps = [src] + [os.path.join(_CSRC, h) for h in ("spl_scan_words.h", "spl_scan_masks.h", "spl_scan.h", "spl_common.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-DSPL_WORD_TWO_ONE=0" if broken == "full" else f"-DSPL_WORDS_SIM_BREAK={broken}", "-o", out, src])
    return out


_libs = {}


def lib(broken=0):
    if broken not in _libs:
        L = ctypes.CDLL(build(broken))
        L.ws_create.restype = ctypes.c_void_p
        L.ws_create.argtypes = [ctypes.c_char_p, ctypes.c_int]
        L.ws_destroy.argtypes = [ctypes.c_void_p]
        L.ws_one.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        for s in SWEEPS:
            getattr(L, "ws_sweep_" + s).argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        _libs[broken] = L
    return _libs[broken]


STATS = ["cases", "text_done", "two_taken", "mismatch", "two_mismatch", "declined_well_formed", "took_malformed", "guard_violation", "well_formed",
         "malformed", "overlong", "overlong_taken", "chars2", "chars3"]


class WordsSim:
    def __init__(self, table=TABLES[0], broken=0):
        self._L = lib(broken)
        assert self._L.ws_n_stats() == len(STATS)
        with open(os.path.join(_DATA, table), "rb") as f:
            u = f.read()
        self._h = self._L.ws_create(u, len(u))
        if not self._h:
            raise ValueError("bad unicode class table")

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.ws_destroy(self._h)
            self._h = None

    def sweep(self, which, pattern):
        """The counts of one sweep (STATS) for one split pattern."""
        st = np.zeros(len(STATS), dtype=np.uint64)
        getattr(self._L, "ws_sweep_" + which)(self._h, PATTERNS[pattern], st.ctypes.data)
        return dict(zip(STATS, (int(x) for x in st)))

    def one(self, pattern, wp_tw_wn: bytes, ts16=0, i0=64, lo=0, iT=1 << 20):
        """One word: (classify_word_text's WordKinds or None, classify_word's, classify_word_two's or None), each (rec, v0, v1)."""
        assert len(wp_tw_wn) == 12
        out = np.zeros(9, dtype=np.uint32)
        r = self._L.ws_one(self._h, PATTERNS[pattern], wp_tw_wn, ts16, i0, lo, iT, out.ctypes.data)
        o = [tuple(int(x) for x in out[3 * k:3 * k + 3]) for k in range(3)]
        return (o[0] if r & 1 else None), o[1], (o[2] if r & 2 else None)
