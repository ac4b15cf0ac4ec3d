"""ctypes wrapper of tests/hostsim/choice_sim.cpp (TEST TOOL; builds with g++, no GPU needed)."""
import ctypes
import os
import subprocess

import numpy as np

from heal_sim import Vocab  # noqa: F401  (the toy vocabularies' decode tables, as the healing simulation builds them)

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "splintr_amd", "csrc")
WORD_POISON = 0xA5A5A5A5A5A5A5A5
MASK_POISON = 0x5A5A5A5A
WORDS = 2
THEN_FREE, KEEP_FREE, I64 = 1, 2, 4
PIECE = 8192
MUTANTS = {"": [], "lcp": ["-DSPL_CHOICE_MUTANT_LCP"], "eq": ["-DSPL_CHOICE_MUTANT_EQ"]}


def build(mutant=""):
    src = os.path.join(_HERE, "choice_sim.cpp")
    out = os.path.join(_HERE, "libchoice_sim%s.so" % ("_" + mutant if mutant else ""))
    deps = [src] + [os.path.join(_CSRC, f) for f in ("spl_k_choice.h", "spl_k_heal.h", "spl_common.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas"] + MUTANTS[mutant] + ["-o", out, src])
    return out


_libs = {}


def lib(mutant=""):
    if mutant not in _libs:
        L = ctypes.CDLL(build(mutant))
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        L.ch_geometry.argtypes = [vp]
        L.ch_sim.argtypes = [vp, vp, vp, u32, vp, vp, u64, u32, u32, u32, u32, u32, u32, vp, vp, u32] + [vp] * 8
        _libs[mutant] = L
    return _libs[mutant]


def geometry():
    g = np.zeros(8, dtype=np.uint32)
    lib().ch_geometry(g.ctypes.data)
    return dict(zip(["slots", "max_len", "table_bytes", "state_words", "max_end", "piece", "wave", "regs"], g.tolist()))


def run(v, table, *, ids, state, lengths=None, flags=0, end_ids=(), n_words=None, piece=PIECE, v4=None, lanes=64, in_place=False, mask_init=None,
        mutant=""):
    """One call of the kernel's code -> dict(state uint64 [B, 2], mask uint32 [B, n_words], live).  Asserts on the way: every state word and
    live byte written exactly ONCE; every mask word of a written row exactly once (with KEEP_FREE a row that is not constrained after the
    call not at all); nothing else written (poisoned destinations, a spare row behind each); no canary damaged, no 16-byte store off its
    alignment.  v4 None: 16-byte stores whenever the row width allows them."""
    ids = np.ascontiguousarray(ids)
    assert ids.ndim == 2 and ids.dtype in (np.int32, np.int64, np.uint32)
    if ids.dtype == np.int64:
        flags |= I64
    B, K = ids.shape
    n_words = v.min_words if n_words is None else n_words
    v4 = (n_words % 4 == 0) if v4 is None else v4
    lens = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.int32)
    table = np.ascontiguousarray(table, dtype=np.uint8)
    ends = np.array(list(end_ids), dtype=np.uint32)
    st_in = np.ascontiguousarray(state, dtype=np.uint64).copy().reshape(B, WORDS)
    if in_place:
        st_in = np.concatenate([st_in, np.full((1, WORDS), WORD_POISON, dtype=np.uint64)])
    st_out = st_in if in_place else np.full((B + 1, WORDS), WORD_POISON, dtype=np.uint64)
    st_w = np.zeros((B + 1, WORDS), dtype=np.uint8)
    mask = np.full((B + 1, n_words), MASK_POISON, dtype=np.uint32)
    if mask_init is not None:
        mask[:B] = mask_init
    mask_w = np.zeros((B + 1, n_words), dtype=np.uint8)
    live = np.full(B + 1, 0x5A, dtype=np.uint8)
    live_w = np.zeros(B + 1, dtype=np.uint8)
    stats = np.zeros(2, dtype=np.uint64)
    ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data
    rc = lib(mutant).ch_sim(v.off.ctypes.data, v.blob.ctypes.data, v.present.ctypes.data, v.max_id, ptr(ids), ptr(lens), B, K, flags, n_words,
                            piece, int(v4), len(ends), ptr(ends), table.ctypes.data, lanes, st_in.ctypes.data, st_out.ctypes.data,
                            st_w.ctypes.data, mask.ctypes.data, mask_w.ctypes.data, live.ctypes.data, live_w.ctypes.data, stats.ctypes.data)
    assert rc == 0, rc
    assert (st_w[:B] == 1).all() and (st_w[B] == 0).all() and (st_out[B] == WORD_POISON).all(), "a state word not written exactly once"
    assert (live_w[:B] == 1).all() and live_w[B] == 0 and live[B] == 0x5A, "a live byte not written exactly once"
    skip = (live[:B] == 0) if flags & KEEP_FREE else np.zeros(B, dtype=bool)
    assert (mask_w[:B][~skip] == 1).all(), "a mask word of a written row not written exactly once"
    assert (mask_w[:B][skip] == 0).all(), "KEEP_FREE: a row that is not constrained was written"
    assert (mask_w[B] == 0).all() and (mask[B] == MASK_POISON).all(), "written behind the last row"
    assert stats[0] == 0, "canary damage or a 16-byte store off its alignment"
    return dict(state=st_out[:B].copy(), mask=mask[:B].copy(), live=live[:B].copy(), n_ordinary=int(stats[1]))
