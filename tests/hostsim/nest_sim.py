"""ctypes wrapper of tests/hostsim/nest_sim.cpp (TEST TOOL; builds with g++, no GPU needed)."""
import ctypes
import os
import subprocess

import numpy as np

from heal_sim import Vocab  # noqa: F401  (the toy vocabularies' decode tables, as the healing simulation builds them)
from nest_cases import TooSmall

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "splintr_amd", "csrc")
WORD_POISON = 0xA5A5A5A5A5A5A5A5
MASK_POISON = 0x5A5A5A5A
KEEP_FREE, I64 = 2, 4
S_BLOCK = 256
STATE_WORDS = 5
MUTANTS = {"": [], "pop": ["-DSPL_NEST_MUTANT_POP"], "end": ["-DSPL_NEST_MUTANT_END"], "dep": ["-DSPL_NEST_MUTANT_DEP"]}


def build(mutant=""):
    src = os.path.join(_HERE, "nest_sim.cpp")
    out = os.path.join(_HERE, "libnest_sim%s.so" % ("_" + mutant if mutant else ""))
    deps = [src] + [os.path.join(_CSRC, f) for f in ("spl_k_nest.h", "spl_k_dfa.h", "spl_k_heal.h", "spl_common.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas"] + MUTANTS[mutant] + ["-o", out, src])
    return out


_libs = {}


def lib(mutant=""):
    if mutant not in _libs:
        L = ctypes.CDLL(build(mutant))
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        L.ns_geometry.argtypes = [vp]
        L.ns_index_sim.argtypes = [vp, vp, vp, u32, vp, u32, u32, u32, u32, u32, u32] + [vp] * 9
        L.ns_sim.argtypes = [vp, vp, vp, u32, vp, vp, u64, u32, u32, u32, u32, u32, vp, u32, vp, u32, u32, vp, vp, vp, u32, vp, u32] + [vp] * 8
        _libs[mutant] = L
    return _libs[mutant]


def geometry():
    g = np.zeros(8, dtype=np.uint32)
    lib().ns_geometry(g.ctypes.data)
    return dict(zip(["max_depth", "state_words", "max_ret", "push", "pop", "piece", "max_states", "max_end"], g.tolist()))


def stride_of(n_words):
    return (n_words + 3) // 4 * 4


def index(v, table, n_states, n_ret, n_words=None, *, dep_cap=None, lanes=64, s_block=S_BLOCK, mutant=""):
    """The index build of the kernels' code -> (rows uint32 [S, stride], some uint8 [S], dep_off uint32 [S + 1], dep_ids uint32 [n_dep]).
    dep_cap None: the exact size (found by a first build that is refused).  Asserts on the way: every word of every row, every some byte,
    every dep_off and every dep entry stored exactly ONCE, nothing else written -- nothing at all behind dep_cap -- and no canary damaged.
    Raises TooSmall(n_dep) where dep_cap does not hold the entries."""
    n_words = v.min_words if n_words is None else n_words
    table = np.ascontiguousarray(table, dtype=np.uint8)
    assert table.size == n_states * 769 + n_ret * 32
    if dep_cap is None:
        try:
            return index(v, table, n_states, n_ret, n_words, dep_cap=0, lanes=lanes, s_block=s_block, mutant=mutant)
        except TooSmall as e:
            dep_cap = e.args[0]
    stride = stride_of(n_words)
    rows = np.full((n_states + 1, stride), MASK_POISON, dtype=np.uint32)
    rows_w = np.zeros((n_states + 1, stride), dtype=np.uint8)
    dep_off = np.full(n_states + 2, MASK_POISON, dtype=np.uint32)
    dep_off_w = np.zeros(n_states + 2, dtype=np.uint8)
    dep_ids = np.full(dep_cap + 4, MASK_POISON, dtype=np.uint32)
    dep_w = np.zeros(dep_cap + 4, dtype=np.uint8)
    some = np.full(n_states + 1, 0x5A, dtype=np.uint8)
    some_w = np.zeros(n_states + 1, dtype=np.uint8)
    stats = np.zeros(3, dtype=np.uint64)
    rc = lib(mutant).ns_index_sim(v.off.ctypes.data, v.blob.ctypes.data, v.present.ctypes.data, v.max_id, table.ctypes.data, n_states, n_ret, n_words,
                                  lanes, s_block, dep_cap, rows.ctypes.data, rows_w.ctypes.data, dep_off.ctypes.data, dep_off_w.ctypes.data,
                                  dep_ids.ctypes.data, dep_w.ctypes.data, some.ctypes.data, some_w.ctypes.data, stats.ctypes.data)
    assert rc in (0, -4), rc
    assert stats[0] == 0, "canary damage or a store outside the index"
    assert (rows_w[:n_states] == 1).all(), "an index word not stored exactly once"
    assert (some_w[:n_states] == 1).all(), "a some byte not stored exactly once"
    assert (dep_off_w[:n_states + 1] == 1).all() and dep_off_w[n_states + 1] == 0, "a dep_off entry not stored exactly once"
    assert (rows_w[n_states] == 0).all() and (rows[n_states] == MASK_POISON).all() and some_w[n_states] == 0 and some[n_states] == 0x5A, "written behind the index"
    n_dep = int(stats[2])
    assert int(dep_off[n_states]) == n_dep
    if rc == -4:
        assert n_dep > dep_cap and (dep_w == 0).all() and (dep_ids == MASK_POISON).all(), "a refused build wrote dependent entries"
        raise TooSmall(n_dep)
    assert (dep_w[:n_dep] == 1).all() and (dep_w[n_dep:] == 0).all() and (dep_ids[n_dep:] == MASK_POISON).all(), "a dep entry not stored exactly once"
    return rows[:n_states].copy(), some[:n_states].copy(), dep_off[:n_states + 1].copy(), dep_ids[:n_dep].copy()


_index_cache = {}


def run(v, table, n_states, n_ret, *, ids, state, max_depth=64, lengths=None, flags=0, end_ids=(), n_words=None, v4=None, lanes=64, in_place=False,
        mask_init=None, mutant="", the_index=None):
    """One call of the step's code -> dict(state uint64 [B, 5], mask uint32 [B, n_words], live).  The index is the one the kernels' code
    builds (kept per table).  Asserts on the way: every state word and live byte written exactly ONCE; every mask word of a written row
    exactly once (with KEEP_FREE a row that is not constrained after the call not at all); nothing else written (poisoned destinations,
    a spare row behind each); no canary damaged, no 16-byte store off its alignment."""
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
        key = (id(v), table.tobytes(), n_states, n_ret, n_words, mutant)
        if key not in _index_cache:
            _index_cache[key] = index(v, table, n_states, n_ret, n_words, lanes=64, mutant=mutant)
        the_index = _index_cache[key]
    rows, some = np.ascontiguousarray(the_index[0], dtype=np.uint32), np.ascontiguousarray(the_index[1], dtype=np.uint8)
    dep_off = np.ascontiguousarray(the_index[2], dtype=np.uint32)
    dep_ids = np.ascontiguousarray(np.concatenate([the_index[3], np.zeros(1, dtype=np.uint32)]), dtype=np.uint32)
    dep_cap = len(the_index[3])
    ends = np.array(list(end_ids), dtype=np.uint32)
    st_in = np.ascontiguousarray(state, dtype=np.uint64).copy().reshape(B, STATE_WORDS)
    if in_place:
        st_in = np.concatenate([st_in, np.full((1, STATE_WORDS), WORD_POISON, dtype=np.uint64)])
    st_out = st_in if in_place else np.full((B + 1, STATE_WORDS), WORD_POISON, dtype=np.uint64)
    st_w = np.zeros((B + 1, STATE_WORDS), dtype=np.uint8)
    mask = np.full((B + 1, n_words), MASK_POISON, dtype=np.uint32)
    if mask_init is not None:
        mask[:B] = mask_init
    mask_w = np.zeros((B + 1, n_words), dtype=np.uint8)
    live = np.full(B + 1, 0x5A, dtype=np.uint8)
    live_w = np.zeros(B + 1, dtype=np.uint8)
    stats = np.zeros(2, dtype=np.uint64)
    ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data
    rc = lib(mutant).ns_sim(v.off.ctypes.data, v.blob.ctypes.data, v.present.ctypes.data, v.max_id, ptr(ids), ptr(lens), B, K, flags, n_words,
                            int(v4), len(ends), ptr(ends), max_depth, table.ctypes.data, n_states, n_ret, rows.ctypes.data, dep_off.ctypes.data,
                            dep_ids.ctypes.data, dep_cap, some.ctypes.data, lanes, st_in.ctypes.data, st_out.ctypes.data, st_w.ctypes.data,
                            mask.ctypes.data, mask_w.ctypes.data, live.ctypes.data, live_w.ctypes.data, stats.ctypes.data)
    assert rc == 0, rc
    assert (st_w[:B] == 1).all() and (st_w[B] == 0).all() and (st_out[B] == WORD_POISON).all(), "a state word not written exactly once"
    assert (live_w[:B] == 1).all() and live_w[B] == 0 and live[B] == 0x5A, "a live byte not written exactly once"
    skip = (live[:B] == 0) if flags & KEEP_FREE else np.zeros(B, dtype=bool)
    assert (mask_w[:B][~skip] == 1).all(), "a mask word of a written row not written exactly once"
    assert (mask_w[:B][skip] == 0).all(), "KEEP_FREE: a row that is not constrained was written"
    assert (mask_w[B] == 0).all() and (mask[B] == MASK_POISON).all(), "written behind the last row"
    assert stats[0] == 0, "canary damage or a 16-byte store off its alignment"
    return dict(state=st_out[:B].copy(), mask=mask[:B].copy(), live=live[:B].copy(), n_ordinary=int(stats[1]))
