"""ctypes wrapper of tests/hostsim/jump_sim.cpp (TEST TOOL; builds with g++, no GPU needed)."""
import ctypes
import os
import subprocess

import numpy as np

import dfa_sim
from heal_sim import Vocab  # noqa: F401  (the toy vocabularies' decode tables, as the healing simulation builds them)

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "splintr_amd", "csrc")
WORD_POISON = dfa_sim.WORD_POISON
MASK_POISON = dfa_sim.MASK_POISON
ID_POISON = -0x5A5A5A5B
KEEP_FREE, I64 = 2, 4
MAX_BYTES = MAX_IDS = 64
PER_STATE = 64 * 4 + 1 + 1 + 64
MUTANTS = {"": [], "accept": ["-DSPL_DFA_JUMP_MUTANT_ACCEPT"], "nowalk": ["-DSPL_DFA_JUMP_MUTANT_NOWALK"]}


def build(mutant=""):
    src = os.path.join(_HERE, "jump_sim.cpp")
    out = os.path.join(_HERE, "libjump_sim%s.so" % ("_" + mutant if mutant else ""))
    deps = [src] + [os.path.join(_CSRC, f) for f in ("spl_k_dfa_jump.h", "spl_k_dfa.h", "spl_k_heal.h", "spl_common.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas"] + MUTANTS[mutant] + ["-o", out, src])
    return out


_libs = {}


def lib(mutant=""):
    if mutant not in _libs:
        L = ctypes.CDLL(build(mutant))
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        L.jm_geometry.argtypes = [vp]
        L.jm_runs_sim.argtypes = [vp, u32, u32] + [vp] * 7
        L.jm_scatter_sim.argtypes = [vp, vp, u64, u32, u32] + [vp] * 5
        L.jm_sim.argtypes = [vp, vp, vp, u32, vp, vp, u64, u32, u32, u32, u32, u32, vp, vp, u32, vp, vp, u32] + [vp] * 8 + [u32] + [vp] * 5
        _libs[mutant] = L
    return _libs[mutant]


def geometry():
    g = np.zeros(4, dtype=np.uint32)
    lib().jm_geometry(g.ctypes.data)
    return dict(zip(["max_bytes", "max_ids", "index_bytes_per_state", "none"], g.tolist()))


def runs(table, n_states, *, lanes=64, mutant=""):
    """The force and runs launches of the kernels' code -> (run uint8 [S, 64], run_len uint8 [S], force uint32 [S]).  Asserts on the way:
    every force word, every byte of every run row and every length stored exactly ONCE, nothing else written, no canary damaged."""
    table = np.ascontiguousarray(table, dtype=np.uint8)
    assert table.size == n_states * 513
    S = n_states
    force = np.full(S + 1, MASK_POISON, dtype=np.uint32)
    force_w = np.zeros(S + 1, dtype=np.uint8)
    run = np.full((S + 1, MAX_BYTES), 0x5A, dtype=np.uint8)
    run_w = np.zeros((S + 1, MAX_BYTES), dtype=np.uint8)
    run_len = np.full(S + 1, 0x5A, dtype=np.uint8)
    len_w = np.zeros(S + 1, dtype=np.uint8)
    stats = np.zeros(2, dtype=np.uint64)
    rc = lib(mutant).jm_runs_sim(table.ctypes.data, S, lanes, force.ctypes.data, force_w.ctypes.data, run.ctypes.data, run_w.ctypes.data,
                                 run_len.ctypes.data, len_w.ctypes.data, stats.ctypes.data)
    assert rc == 0, rc
    assert (force_w[:S] == 1).all() and (run_w[:S] == 1).all() and (len_w[:S] == 1).all(), "a word or a byte not stored exactly once"
    assert force_w[S] == 0 and (run_w[S] == 0).all() and len_w[S] == 0 and (run[S] == 0x5A).all() and run_len[S] == 0x5A, "written behind the index"
    assert stats[0] == 0, "canary damage or a store outside the index"
    return run[:S].copy(), run_len[:S].copy(), force[:S].copy()


def scatter(csr, off, n_states, *, cap=None, lanes=64):
    """The scatter launch -> (ids uint32 [S, 64], n_ids uint8 [S]); every id and every count stored exactly once."""
    csr = np.ascontiguousarray(csr, dtype=np.uint32)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    assert off.size == n_states + 1
    S = n_states
    ids = np.full((S + 1, MAX_IDS), MASK_POISON, dtype=np.uint32)
    ids_w = np.zeros((S + 1, MAX_IDS), dtype=np.uint8)
    n_ids = np.full(S + 1, 0x5A, dtype=np.uint8)
    n_w = np.zeros(S + 1, dtype=np.uint8)
    stats = np.zeros(2, dtype=np.uint64)
    padded = np.concatenate([csr, np.zeros(1, dtype=np.uint32)])
    rc = lib().jm_scatter_sim(padded.ctypes.data, off.ctypes.data, len(csr) if cap is None else cap, S, lanes, ids.ctypes.data, ids_w.ctypes.data,
                              n_ids.ctypes.data, n_w.ctypes.data, stats.ctypes.data)
    assert rc == 0, rc
    assert (ids_w[:S] == 1).all() and (n_w[:S] == 1).all(), "an id or a count not stored exactly once"
    assert (ids_w[S] == 0).all() and n_w[S] == 0 and stats[0] == 0
    return ids[:S].copy(), n_ids[:S].copy()


def run(v, table, n_states, *, ids, state, jump_index, row_len_out=16, lengths=None, flags=0, end_ids=(), n_words=None, v4=None, lanes=64, in_place=False,
        mask_init=None, mutant="", the_index=None):
    """One call of the jump step's code -> dict(state, mask, live, forced int32 [B, row_len_out], forced_len int32 [B]).  Asserts on the
    way what dfa_sim.run asserts of the step, and: every forced_len written exactly ONCE; the entries of forced below forced_len exactly
    once, those at and beyond it not at all (they keep their poison); nothing written behind the last row."""
    ids = np.ascontiguousarray(ids)
    assert ids.ndim == 2 and ids.dtype in (np.int32, np.int64, np.uint32)
    if ids.dtype == np.int64:
        flags |= I64
    B, K = ids.shape
    n_words = v.min_words if n_words is None else n_words
    v4 = (n_words % 4 == 0) if v4 is None else v4
    lens = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.int32)
    table = np.ascontiguousarray(table, dtype=np.uint8)
    if the_index is None:
        key = (id(v), table.tobytes(), n_states, n_words, "")
        if key not in dfa_sim._index_cache:
            dfa_sim._index_cache[key] = dfa_sim.index(v, table, n_states, n_words, lanes=64)
        the_index = dfa_sim._index_cache[key]
    rows, some = np.ascontiguousarray(the_index[0], dtype=np.uint32), np.ascontiguousarray(the_index[1], dtype=np.uint8)
    jump_index = np.ascontiguousarray(jump_index, dtype=np.uint8)
    assert jump_index.size == n_states * PER_STATE and jump_index.ctypes.data % 4 == 0
    ends = np.array(list(end_ids), dtype=np.uint32)
    st_in = np.ascontiguousarray(state, dtype=np.uint64).copy().reshape(B)
    if in_place:
        st_in = np.concatenate([st_in, np.full(1, WORD_POISON, dtype=np.uint64)])
    st_out = st_in if in_place else np.full(B + 1, WORD_POISON, dtype=np.uint64)
    st_w = np.zeros(B + 1, dtype=np.uint8)
    mask = np.full((B + 1, n_words), MASK_POISON, dtype=np.uint32)
    if mask_init is not None:
        mask[:B] = mask_init
    mask_w = np.zeros((B + 1, n_words), dtype=np.uint8)
    live = np.full(B + 1, 0x5A, dtype=np.uint8)
    live_w = np.zeros(B + 1, dtype=np.uint8)
    forced = np.full((B + 1, row_len_out), ID_POISON, dtype=np.int32)
    forced_w = np.zeros((B + 1, row_len_out), dtype=np.uint8)
    flen = np.full(B + 1, ID_POISON, dtype=np.int32)
    flen_w = np.zeros(B + 1, dtype=np.uint8)
    stats = np.zeros(2, dtype=np.uint64)
    ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data
    rc = lib(mutant).jm_sim(v.off.ctypes.data, v.blob.ctypes.data, v.present.ctypes.data, v.max_id, ptr(ids), ptr(lens), B, K, flags, n_words,
                            int(v4), len(ends), ptr(ends), table.ctypes.data, n_states, rows.ctypes.data, some.ctypes.data, lanes,
                            st_in.ctypes.data, st_out.ctypes.data, st_w.ctypes.data, mask.ctypes.data, mask_w.ctypes.data, live.ctypes.data,
                            live_w.ctypes.data, jump_index.ctypes.data, row_len_out, forced.ctypes.data, forced_w.ctypes.data, flen.ctypes.data,
                            flen_w.ctypes.data, stats.ctypes.data)
    assert rc == 0, rc
    assert (st_w[:B] == 1).all() and st_w[B] == 0 and st_out[B] == WORD_POISON, "a state word not written exactly once"
    assert (live_w[:B] == 1).all() and live_w[B] == 0 and live[B] == 0x5A, "a live byte not written exactly once"
    skip = (live[:B] == 0) if flags & KEEP_FREE else np.zeros(B, dtype=bool)
    assert (mask_w[:B][~skip] == 1).all(), "a mask word of a written row not written exactly once"
    assert (mask_w[:B][skip] == 0).all(), "KEEP_FREE: a row that is not constrained was written"
    assert (mask_w[B] == 0).all() and (mask[B] == MASK_POISON).all(), "written behind the last row"
    assert (flen_w[:B] == 1).all() and flen_w[B] == 0 and flen[B] == ID_POISON, "a forced_len not written exactly once"
    assert ((flen[:B] >= 0) & (flen[:B] <= row_len_out)).all(), "a forced_len outside 0 .. row_len_out"
    below = np.arange(row_len_out)[None, :] < flen[:B, None]
    assert (forced_w[:B][below] == 1).all(), "an emitted id not written exactly once"
    assert (forced_w[:B][~below] == 0).all() and (forced[:B][~below] == ID_POISON).all(), "an entry at or beyond forced_len was written"
    assert (forced_w[B] == 0).all() and (forced[B] == ID_POISON).all(), "written behind the last row of forced ids"
    assert stats[0] == 0, "canary damage, a 16-byte store off its alignment or an emitted id outside its row"
    return dict(state=st_out[:B].copy(), mask=mask[:B].copy(), live=live[:B].copy(), forced=forced[:B].copy(), forced_len=flen[:B].copy(),
                n_ordinary=int(stats[1]))
