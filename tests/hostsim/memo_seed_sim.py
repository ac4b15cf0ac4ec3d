"""ctypes wrapper of tests/hostsim/memo_seed_sim.cpp (TEST TOOL; builds with g++, no GPU needed): the chunk memo's seed -- where the
product's host code puts the vocabulary's keys in a new memo -- and the decoder's view of the vocabulary."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_DATA = os.path.join(_ROOT, "splintr_amd", "data")
_CSRC = os.path.join(_ROOT, "splintr_amd", "csrc")
_LIB = os.path.join(_HERE, "libmemoseedsim.so")
_REG = {"cl100k_base": ("cl100k_base.splv", 0), "o200k_base": ("o200k_base.splv", 1),
        "llama3": ("llama3.splv", 1), "deepseek_v3": ("deepseek_v3.splv", 1), "mistral_v3": ("mistral_v3.splv", 2)}


def build():
    srcs = [os.path.join(_HERE, "memo_seed_sim.cpp"), os.path.join(_CSRC, "spl_tables.cpp")]
    deps = srcs + [os.path.join(_CSRC, h) for h in ("spl_common.h", "spl_lookup.h", "spl_tables.h")]
    if not os.path.exists(_LIB) or any(os.path.getmtime(d) > os.path.getmtime(_LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", _LIB] + srcs)
    return _LIB


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build())
        L.ms_create.restype = ctypes.c_void_p
        L.ms_create.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
        L.ms_destroy.argtypes = [ctypes.c_void_p]
        L.ms_plan.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
        L.ms_records.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32] + [ctypes.c_void_p] * 4
        L.ms_n_ids.restype = ctypes.c_uint32
        L.ms_n_ids.argtypes = [ctypes.c_void_p]
        L.ms_token_bytes_total.restype = ctypes.c_uint32
        L.ms_token_bytes_total.argtypes = [ctypes.c_void_p]
        L.ms_tokens.argtypes = [ctypes.c_void_p] * 4
        _lib = L
    return _lib


class MemoSeedSim:
    def __init__(self, name=None, path=None, pattern_id=0):
        if path is None:
            fn, pattern_id = _REG[name]
            path = os.path.join(_DATA, fn)
        err = ctypes.create_string_buffer(256)
        self._h = lib().ms_create(str(path).encode(), os.path.join(_DATA, "unicode_classes.bin").encode(), pattern_id, err, 256)
        if not self._h:
            raise ValueError(err.value.decode())

    def __del__(self):
        if getattr(self, "_h", None):
            lib().ms_destroy(self._h)
            self._h = None

    def tokens(self):
        """{id: bytes} of every id whose bytes are a key of the encoder (in the key space the kernels see: raw bytes)."""
        n = lib().ms_n_ids(self._h)
        off = np.zeros(n + 1, dtype=np.uint32)
        blob = np.zeros(max(1, lib().ms_token_bytes_total(self._h)), dtype=np.uint8)
        present = np.zeros(n, dtype=np.uint8)
        lib().ms_tokens(self._h, off.ctypes.data, blob.ctypes.data, present.ctypes.data)
        raw = blob.tobytes()
        return {i: raw[off[i]:off[i + 1]] for i in range(n) if present[i] == 1 and off[i + 1] > off[i]}

    def plan(self, bits, long_bits):
        """The seed of a memo of 2^bits and 2^long_bits entries: (placed, left out), and per table a dict of arrays -- slot, id, n, key
        (the records), first / second (the key's candidate slots as the probe computes them), probed (the vocabulary's whole-chunk probe)."""
        st = np.zeros(4, dtype=np.uint64)
        lib().ms_plan(self._h, bits, long_bits, st.ctypes.data)
        tabs = []
        for lng, cnt, mask in ((0, int(st[2]), (1 << bits) - 1), (1, int(st[3]), (1 << long_bits) - 1 if long_bits else 0)):
            rw = 18 if lng else 10
            recs = np.zeros((max(cnt, 1), rw), dtype=np.uint32)
            first, second, probed = (np.zeros(max(cnt, 1), dtype=np.uint32) for _ in range(3))
            if cnt:
                lib().ms_records(self._h, lng, mask, recs.ctypes.data, first.ctypes.data, second.ctypes.data, probed.ctypes.data)
            recs = recs[:cnt]
            tabs.append({"slot": recs[:, 0], "id": recs[:, 1] & 0xFFFFFF, "n": recs[:, 1] >> 24, "key": recs[:, 2:],
                         "first": first[:cnt], "second": second[:cnt], "probed": probed[:cnt], "mask": mask})
        return (int(st[0]), int(st[1])), tabs
