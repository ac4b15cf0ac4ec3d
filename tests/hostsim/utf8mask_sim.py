"""ctypes wrapper of tests/hostsim/utf8mask_sim.cpp (TEST TOOL; builds with g++, no GPU needed)."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "splintr_amd", "csrc")
MASK_POISON = 0x5A5A5A5A
ROWS = 17
AND = 1
FREE = 8


def build():
    src = os.path.join(_HERE, "utf8mask_sim.cpp")
    out = os.path.join(_HERE, "libutf8mask_sim.so")
    deps = [src] + [os.path.join(_CSRC, f) for f in ("spl_k_utf8mask.h", "spl_k_heal.h", "spl_k_stream.h", "spl_k_decode_dev.h", "spl_common.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", out, src])
    return out


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build())
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        L.um_sim_step.restype = L.um_sim_class.restype = L.um_sim_token_classes.restype = u32
        L.um_sim_step.argtypes = [u32, u32]
        L.um_sim_class.argtypes = [u64]
        L.um_sim_token_classes.argtypes = [ctypes.c_char_p, u32]
        L.um_geometry.argtypes = [vp]
        L.um_sim_table.argtypes = [vp, vp, u32, vp, vp, u32, vp, vp, u32, vp, vp, vp]
        L.um_sim_mask.argtypes = [vp, u32, vp, u64, u32, u32, u32, u32, vp, vp, vp, vp, vp]
        _lib = L
    return _lib


def step(s, x):
    return lib().um_sim_step(s, x)


def state_class(word):
    return lib().um_sim_class(int(word))


def token_classes(b):
    return lib().um_sim_token_classes(bytes(b), len(b))


class Vocab:
    """The decode tables of a toy vocabulary as the library holds them: vocab {id: bytes} is the vocabulary proper, specials {id: bytes} the
    special map (an id of both is a vocabulary id); the dense table runs to the vocabulary's largest id, specials fill its holes, the
    specials beyond it lie in a sorted side table."""

    def __init__(self, vocab, specials=None):
        specials = specials or {}
        self.max_id = max(vocab)
        off, blob = [0], b""
        present = np.zeros(self.max_id // 32 + 1, dtype=np.uint32)
        sp_bits = np.zeros(self.max_id // 32 + 1, dtype=np.uint32)
        for i in range(self.max_id + 1):
            if i in vocab:
                blob += vocab[i]
                present[i >> 5] |= np.uint32(1 << (i & 31))
            elif i in specials:
                blob += specials[i]
                sp_bits[i >> 5] |= np.uint32(1 << (i & 31))
            off.append(len(blob))
        far = sorted(i for i in specials if i > self.max_id)
        sp_off = []
        for i in far:
            sp_off.append(len(blob))
            blob += specials[i]
        sp_off.append(len(blob))
        self.off = np.array(off, dtype=np.uint32)
        self.blob = np.frombuffer(blob + b"\0", dtype=np.uint8).copy()
        self.present, self.sp_bits = present, sp_bits
        self.sp_ids = np.array(far + [0], dtype=np.uint32)
        self.sp_off = np.array(sp_off, dtype=np.uint32)
        self.n_sp = len(far)
        self.min_words = max([self.max_id] + far) // 32 + 1
        self.stride = (self.min_words + 3) & ~3


def table(v):
    """The class table uint32 [17, stride] as k_utf8_table's code builds it.  Asserts: every word written exactly once, no canary damaged."""
    rows = np.full((ROWS, v.stride), MASK_POISON, dtype=np.uint32)
    rows_w = np.zeros((ROWS, v.stride), dtype=np.uint8)
    stats = np.zeros(2, dtype=np.uint64)
    rc = lib().um_sim_table(v.off.ctypes.data, v.blob.ctypes.data, v.max_id, v.sp_ids.ctypes.data, v.sp_off.ctypes.data, v.n_sp,
                            v.sp_bits.ctypes.data, v.present.ctypes.data, v.stride, rows.ctypes.data, rows_w.ctypes.data, stats.ctypes.data)
    assert rc == 0, rc
    assert (rows_w == 1).all(), "a word of the table not written exactly once"
    assert stats[0] == 0, "canary damage"
    return rows


def run(rows, words, *, skip=False, and_into=None, n_words, per=1, want_live=True):
    """One step of k_utf8_mask's code over the table -> (mask uint32 [B, n_words], live uint8 [B]).  Asserts on the way: every word of a row
    written exactly once (with and_into: read once and written once, a stalled row neither), every live byte once, nothing behind the last
    row."""
    state = np.ascontiguousarray(words, dtype=np.uint64)
    B = len(state)
    mask = np.full((B + 1, n_words), MASK_POISON, dtype=np.uint32)
    if and_into is not None:
        mask[:B] = and_into
    mask_w = np.zeros((B + 1, n_words), dtype=np.uint8)
    mask_r = np.zeros((B + 1, n_words), dtype=np.uint8)
    live = np.full(B + 1, 0x5A, dtype=np.uint8)
    live_w = np.zeros(B + 1, dtype=np.uint8)
    rows = np.ascontiguousarray(rows)
    rc = lib().um_sim_mask(rows.ctypes.data, rows.shape[1], state.ctypes.data, B, int(skip), AND if and_into is not None else 0, n_words, per,
                           mask.ctypes.data, mask_w.ctypes.data, mask_r.ctypes.data, live.ctypes.data if want_live else None,
                           live_w.ctypes.data if want_live else None)
    assert rc == 0, rc
    stalled = np.array([state_class(w) == FREE for w in state], dtype=bool)
    touched = ~stalled if and_into is not None else np.ones(B, dtype=bool)
    assert (mask_w[:B][touched] == 1).all() and (mask_w[:B][~touched] == 0).all(), "a mask word not written exactly once"
    assert (mask_r[:B] == (mask_w[:B] if and_into is not None else 0)).all(), "a mask word read that should not be, or not read once"
    assert (mask_w[B] == 0).all() and (mask[B] == MASK_POISON).all(), "written behind the last row"
    if want_live:
        assert (live_w[:B] == 1).all() and live_w[B] == 0 and live[B] == 0x5A, "a live byte not written exactly once"
    else:
        assert (live_w == 0).all()
    return mask[:B].copy(), live[:B].copy()
