"""ctypes wrapper of tests/hostsim/draft_sim.cpp (TEST TOOL; builds with g++, no GPU needed)."""
import ctypes
import os
import subprocess

import numpy as np

import dfa_sim
import nest_sim
from heal_sim import Vocab  # noqa: F401  (the toy vocabularies' decode tables, as the healing simulation builds them)

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "splintr_amd", "csrc")
WORD_POISON = 0xA5A5A5A5A5A5A5A5
MASK_POISON = 0x5A5A5A5A
KEEP_FREE, I64 = 2, 4
GUARD = 8                                                              # entries in front of and behind a parent row
MUTANTS = {"": [], "order": ["-DSPL_DRAFT_MUTANT_ORDER"], "ok": ["-DSPL_DRAFT_MUTANT_OK"], "done": ["-DSPL_DRAFT_MUTANT_DONE"]}


def build(mutant=""):
    src = os.path.join(_HERE, "draft_sim.cpp")
    out = os.path.join(_HERE, "libdraft_sim%s.so" % ("_" + mutant if mutant else ""))
    deps = [src] + [os.path.join(_CSRC, f) for f in ("spl_k_draft.h", "spl_k_nest.h", "spl_k_dfa.h", "spl_k_heal.h", "spl_common.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas"] + MUTANTS[mutant] + ["-o", out, src])
    return out


_libs = {}


def lib(mutant=""):
    if mutant not in _libs:
        L = ctypes.CDLL(build(mutant))
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        L.dr_geometry.argtypes = [vp]
        L.dr_dfa_sim.argtypes = [vp, vp, vp, u32, vp, vp, vp, u32, u64, u32, u32, u32, u32, u32, vp, vp, u32, vp, vp, u32] + [vp] * 10
        L.dr_nest_sim.argtypes = [vp, vp, vp, u32, vp, vp, vp, u32, u64, u32, u32, u32, u32, u32, vp, u32, vp, u32, u32, vp, vp, vp, u32, vp, u32] + [vp] * 10
        _libs[mutant] = L
    return _libs[mutant]


def geometry():
    g = np.zeros(2, dtype=np.uint32)
    lib().dr_geometry(g.ctypes.data)
    return dict(max_nodes=int(g[0]), parent_per_seq=int(g[1]))


def draft(v, kind, table, n_states, n_ret=0, *, ids, state, parent=None, lengths=None, flags=0, end_ids=(), n_words=None, max_depth=64, v4=None, lanes=64,
          mask_init=None, want_live=True, want_state=True, mutant=""):
    """One draft call of the kernels' code, kind "dfa" or "nest" -> dict(mask uint32 [B, 1 + K, n_words], ok uint8 [B, K], live uint8
    [B, 1 + K] or None, state uint64 [B, 1 + K(, 5)] or None).  The index is the one the step's simulation builds.  Asserts on the way:
    every ok byte, and every live byte and state word that is wanted, written exactly ONCE; every mask word of a written row exactly once
    (with KEEP_FREE a row that is not constrained not at all); nothing else written (poisoned destinations, a spare row behind each);
    state_in byte-equal before and after; the parents read between guards that would make an orphan look sound; no canary damaged, no
    16-byte store off its alignment."""
    ids = np.ascontiguousarray(ids)
    assert ids.ndim == 2 and ids.dtype in (np.int32, np.int64, np.uint32)
    if ids.dtype == np.int64:
        flags |= I64
    B, K = ids.shape
    R = 1 + K
    W = 1 if kind == "dfa" else nest_sim.STATE_WORDS
    n_words = v.min_words if n_words is None else n_words
    v4 = (n_words % 4 == 0) if v4 is None else v4
    lens = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.int32)
    table = np.ascontiguousarray(table, dtype=np.uint8)
    ends = np.array(list(end_ids), dtype=np.uint32)
    per_seq, par, par_buf = 0, None, None
    if parent is not None:
        parent = np.ascontiguousarray(parent, dtype=np.int32)
        assert parent.shape in ((K,), (B, K))
        per_seq = int(parent.ndim == 2)
        par_buf = np.full(parent.size + 2 * GUARD, -1, dtype=np.int32)            # (a read outside the row finds a "root": the orphan would pass)
        par_buf[GUARD:GUARD + parent.size] = parent.reshape(-1)
        par = par_buf[GUARD:]
    st_in = np.ascontiguousarray(state, dtype=np.uint64).copy().reshape(B, W)
    st_before = st_in.copy()
    st_out = np.full((B * R + 1, W), WORD_POISON, dtype=np.uint64)
    st_w = np.zeros((B * R + 1, W), dtype=np.uint8)
    mask = np.full((B * R + 1, n_words), MASK_POISON, dtype=np.uint32)
    if mask_init is not None:
        mask[:B * R] = np.asarray(mask_init, dtype=np.uint32).reshape(B * R, n_words)
    mask_w = np.zeros((B * R + 1, n_words), dtype=np.uint8)
    live = np.full(B * R + 1, 0x5A, dtype=np.uint8)
    live_w = np.zeros(B * R + 1, dtype=np.uint8)
    ok = np.full(B * K + 1, 0x5A, dtype=np.uint8)
    ok_w = np.zeros(B * K + 1, dtype=np.uint8)
    stats = np.zeros(2, dtype=np.uint64)
    ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data
    head = (v.off.ctypes.data, v.blob.ctypes.data, v.present.ctypes.data, v.max_id, ptr(ids), ptr(lens), None if par is None else par.ctypes.data, per_seq, B, K,
            flags, n_words, int(v4), len(ends), ptr(ends))
    tail = (lanes, st_in.ctypes.data, st_out.ctypes.data if want_state else None, st_w.ctypes.data, mask.ctypes.data, mask_w.ctypes.data,
            live.ctypes.data if want_live else None, live_w.ctypes.data, ok.ctypes.data, ok_w.ctypes.data, stats.ctypes.data)
    if kind == "dfa":
        key = (id(v), table.tobytes(), n_states, n_words, "")                    # (the step simulation's own cache: one build per table)
        if key not in dfa_sim._index_cache:
            dfa_sim._index_cache[key] = dfa_sim.index(v, table, n_states, n_words)
        rows, some = dfa_sim._index_cache[key]
        rows, some = np.ascontiguousarray(rows, dtype=np.uint32), np.ascontiguousarray(some, dtype=np.uint8)
        rc = lib(mutant).dr_dfa_sim(*head, table.ctypes.data, n_states, rows.ctypes.data, some.ctypes.data, *tail)
    else:
        key = (id(v), table.tobytes(), n_states, n_ret, n_words, "")
        if key not in nest_sim._index_cache:
            nest_sim._index_cache[key] = nest_sim.index(v, table, n_states, n_ret, n_words)
        rows, some, dep_off, dep = nest_sim._index_cache[key]
        rows, some = np.ascontiguousarray(rows, dtype=np.uint32), np.ascontiguousarray(some, dtype=np.uint8)
        dep_off = np.ascontiguousarray(dep_off, dtype=np.uint32)
        dep_ids = np.ascontiguousarray(np.concatenate([dep, np.zeros(1, dtype=np.uint32)]), dtype=np.uint32)
        rc = lib(mutant).dr_nest_sim(*head, max_depth, table.ctypes.data, n_states, n_ret, rows.ctypes.data, dep_off.ctypes.data, dep_ids.ctypes.data, len(dep),
                                     some.ctypes.data, *tail)
    assert rc == 0, rc
    assert (st_in == st_before).all(), "state_in was written"
    if par_buf is not None:
        assert (par_buf[:GUARD] == -1).all() and (par_buf[GUARD + parent.size:] == -1).all()
    n = B * R
    assert (ok_w[:B * K] == 1).all() and ok_w[B * K] == 0 and ok[B * K] == 0x5A, "an ok byte not written exactly once"
    assert (ok[:B * K] <= 1).all()
    if want_state:
        assert (st_w[:n] == 1).all() and (st_w[n] == 0).all() and (st_out[n] == WORD_POISON).all(), "a state word not written exactly once"
    else:
        assert (st_w == 0).all() and (st_out == WORD_POISON).all(), "a state row was written though none was wanted"
    if want_live:
        assert (live_w[:n] == 1).all() and live_w[n] == 0 and live[n] == 0x5A, "a live byte not written exactly once"
    else:
        assert (live_w == 0).all() and (live == 0x5A).all(), "a live byte was written though none was wanted"
    if flags & KEEP_FREE:
        assert want_live, "the simulation tells the rows KEEP_FREE skips by live"
        skip = live[:n] == 0
    else:
        skip = np.zeros(n, dtype=bool)
    assert (mask_w[:n][~skip] == 1).all(), "a mask word of a written row not written exactly once"
    assert (mask_w[:n][skip] == 0).all(), "KEEP_FREE: a row that is not constrained was written"
    assert (mask_w[n] == 0).all() and (mask[n] == MASK_POISON).all(), "written behind the last row"
    assert stats[0] == 0, "canary damage or a 16-byte store off its alignment"
    shape = (B, R) if kind == "dfa" else (B, R, W)
    return dict(mask=mask[:n].reshape(B, R, n_words).copy(), ok=ok[:B * K].reshape(B, K).copy(), live=live[:n].reshape(B, R).copy() if want_live else None,
                state=st_out[:n].reshape(shape).copy() if want_state else None)
