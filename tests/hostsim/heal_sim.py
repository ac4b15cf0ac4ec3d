"""ctypes wrapper of tests/hostsim/heal_sim.cpp (TEST TOOL; builds with g++, no GPU needed)."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "splintr_amd", "csrc")
WORD_POISON = 0xA5A5A5A5A5A5A5A5
MASK_POISON = 0x5A5A5A5A
WORDS = 9
AUTO, KEEP_FREE, I64, PAD_LEFT = 1, 2, 4, 8
MUTANTS = {"": [], "hi": ["-DSPL_HEAL_MUTANT_HI"], "lcp": ["-DSPL_HEAL_MUTANT_LCP"]}


def build(mutant=""):
    src = os.path.join(_HERE, "heal_sim.cpp")
    out = os.path.join(_HERE, "libheal_sim%s.so" % ("_" + mutant if mutant else ""))
    deps = [src] + [os.path.join(_CSRC, f) for f in ("spl_k_heal.h", "spl_common.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas"] + MUTANTS[mutant] + ["-o", out, src])
    return out


_libs = {}


def lib(mutant=""):
    if mutant not in _libs:
        L = ctypes.CDLL(build(mutant))
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        L.hl_geometry.argtypes = [vp]
        L.hl_sim_spw.restype = u32
        L.hl_sim_spw.argtypes = [u64, u32]
        L.hl_sim.argtypes = [vp, vp, vp, u32, ctypes.c_int, vp, vp, u64, u32, u32, u32, u32, u32, u32, u32] + [vp] * 11
        _libs[mutant] = L
    return _libs[mutant]


def geometry():
    g = np.zeros(8, dtype=np.uint32)
    lib().hl_geometry(g.ctypes.data)
    return dict(zip(["wave", "per", "wg_ids", "scr", "state_words", "max_p", "spw_max", "max_part"], g.tolist()))


class Vocab:
    """The decode tables of a toy vocabulary as the library holds them: vocab {id: bytes} is the vocabulary proper, specials {id: bytes} the
    special map (an id of both is a vocabulary id); the dense table runs to the vocabulary's largest id, specials fill its holes."""

    def __init__(self, vocab, specials=None):
        self.vocab = dict(vocab)
        self.max_id = max(self.vocab)
        specials = specials or {}
        off, blob, present = [0], b"", []
        for i in range(self.max_id + 1):
            if i in self.vocab:
                blob += self.vocab[i]
                present.append(1)
            else:
                blob += specials.get(i, b"")
                present.append(0)
            off.append(len(blob))
        self.off = np.array(off, dtype=np.uint32)
        self.blob = np.frombuffer(blob + b"\0", dtype=np.uint8).copy()
        self.present = np.array(present, dtype=np.uint8)
        self.min_words = (self.max_id + 32) // 32


def run(v, *, begin, ids, lengths=None, state=None, flags=0, max_back=0, min_keep=0, n_words=None, lanes=64, spw=None, in_place=False,
        mask_init=None, mutant="", want_n=True):
    """One call of the kernels' code -> dict(state uint64 [B, 9], mask uint32 [B, n_words], live, n_back, n, max_part).  Asserts on the way:
    every state word, live byte and n_back entry written exactly ONCE; every mask word of a written row exactly once (with KEEP_FREE a free
    row not at all); nothing else written (poisoned destinations, a spare row behind each); no canary damaged."""
    ids = np.ascontiguousarray(ids)
    assert ids.ndim == 2 and ids.dtype in (np.int32, np.int64, np.uint32)
    if ids.dtype == np.int64:
        flags |= I64
    B, K = ids.shape
    n_words = v.min_words if n_words is None else n_words
    lens = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.int32)
    st_in = None
    if not begin:
        st_in = np.ascontiguousarray(state, dtype=np.uint64).copy()
        assert st_in.shape == (B, WORDS)
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
    nb = np.full(B + 1, -0x5A5A5A5B, dtype=np.int32)
    nb_w = np.zeros(B + 1, dtype=np.uint8)
    d_n = np.full(2, -7, dtype=np.int32)
    stats = np.zeros(4, dtype=np.uint64)
    ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data
    L = lib(mutant)
    spw = spw or L.hl_sim_spw(B, n_words)
    rc = L.hl_sim(v.off.ctypes.data, v.blob.ctypes.data, v.present.ctypes.data, v.max_id, int(begin), ptr(ids), ptr(lens), B, K, flags,
                  max_back, min_keep, n_words, lanes, spw, ptr(st_in), st_out.ctypes.data, st_w.ctypes.data, mask.ctypes.data,
                  mask_w.ctypes.data, live.ctypes.data, live_w.ctypes.data, nb.ctypes.data if begin else None,
                  nb_w.ctypes.data if begin else None, d_n.ctypes.data if want_n else None, stats.ctypes.data)
    assert rc == 0, rc
    assert (st_w[:B] == 1).all() and (st_w[B] == 0).all() and (st_out[B] == WORD_POISON).all(), "a state word not written exactly once"
    assert (live_w[:B] == 1).all() and live_w[B] == 0 and live[B] == 0x5A, "a live byte not written exactly once"
    if begin:
        assert (nb_w[:B] == 1).all() and nb_w[B] == 0, "an n_back entry not written exactly once"
    else:
        assert (nb_w == 0).all()
    skip = (live[:B] == 0) if flags & KEEP_FREE else np.zeros(B, dtype=bool)
    assert (mask_w[:B][~skip] == 1).all(), "a mask word of a written row not written exactly once"
    assert (mask_w[:B][skip] == 0).all(), "KEEP_FREE: a free row was written"
    assert (mask_w[B] == 0).all() and (mask[B] == MASK_POISON).all(), "written behind the last row"
    assert stats[0] == 0, "canary damage"
    return dict(state=st_out[:B].copy(), mask=mask[:B].copy(), live=live[:B].copy(), n_back=nb[:B].copy(), n=d_n.copy(),
                max_part=int(stats[1]), n_ordinary=int(stats[2]))
