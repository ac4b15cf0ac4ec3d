"""ctypes wrapper of tests/hostsim/seqpack_sim.cpp (TEST TOOL; builds with g++, no GPU needed), and the input layouts the CPU and the
GPU tests of spl_seqpack_device share."""
import ctypes
import os
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "splintr_amd", "csrc")
_LIB = os.path.join(_HERE, "libseqpack_sim.so")
sys.path.insert(0, os.path.dirname(_HERE))
import seqpack_ref as ref  # noqa: E402

I64, PAD_LEFT, KEEP_TAIL, MASK_FIRST = 1, 2, 4, 32


def build():
    src = os.path.join(_HERE, "seqpack_sim.cpp")
    deps = [src] + [os.path.join(_CSRC, f) for f in ("spl_k_seqpack.h", "spl_k_pair.h", "spl_k_collate.h", "spl_k_seqscan.h", "spl_common.h")]
    if not os.path.exists(_LIB) or any(os.path.getmtime(d) > os.path.getmtime(_LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", _LIB, src])
    return _LIB


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build())
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        L.sq_geometry.argtypes = [vp]
        L.sq_work_bytes.argtypes = [u64, u64]
        L.sq_work_bytes.restype = u64
        L.sq_pack.argtypes = [vp] * 5 + [u32] * 10 + [vp] * 12
        _lib = L
    return _lib


def geometry():
    g = np.zeros(8, dtype=np.uint32)
    lib().sq_geometry(g.ctypes.data)
    return dict(zip(["lanes", "vec", "span", "plan_lanes", "lds_max", "pool", "bfd_max_l"], g.tolist()))


def work_bytes(n, R):
    return int(lib().sq_work_bytes(n, R))


class Inputs:
    """n sequences laid out as the device reads them.  form "rows": ids [n, L_in] of int32 / int64 (i64), right or left padded
    (pad_left), lengths int32; form "csr": ids int32 [capacity], off uint64 [n + 1] starting at `lead` (absolute offsets).  labels and
    byte_arrays[k] (lists of lists like seqs, or None) in the same layout.  lengths_override: what the lengths array says instead (bad
    input); the padding of the input holds junk that must never reach an output."""

    def __init__(self, seqs, form="rows", *, i64=False, pad_left=False, L_in=None, labels=None, byte_arrays=(None,) * 4, lead=3,
                 lengths_override=None, off_override=None):
        self.seqs, self.form, self.i64, self.pad_left, self.n = seqs, form, i64, pad_left, len(seqs)
        self.labels, self.byte_arrays = labels, tuple(byte_arrays)
        lens = [len(s) for s in seqs]
        if form == "rows":
            self.L_in = max(lens + [1]) if L_in is None else L_in
            dt = np.int64 if i64 else np.int32

            def lay(vals, dtype, junk):
                if vals is None:
                    return None
                a = np.full((self.n, self.L_in), junk, dtype=dtype)
                for i, s in enumerate(vals):
                    if len(s):
                        if pad_left:
                            a[i, self.L_in - len(s):] = s
                        else:
                            a[i, :len(s)] = s
                return a
            self.ids = lay(seqs, dt, 0x7EADBEEF)
            self.lab = lay(labels, dt, 0x7EADBEEF)
            self.byt = [lay(b, np.uint8, 0xEE) for b in self.byte_arrays]
            self.lengths = np.array(lens if lengths_override is None else lengths_override, dtype=np.int32)
            self.off = None
        else:
            self.L_in = 0
            off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64) + np.uint64(lead)
            cap = int(off[-1]) + 5

            def lay(vals, dtype, junk):
                if vals is None:
                    return None
                a = np.full(cap, junk, dtype=dtype)
                for i, s in enumerate(vals):
                    a[int(off[i]):int(off[i]) + len(s)] = s
                return a
            self.ids = lay(seqs, np.int32, 0x7EADBEEF)
            self.lab = lay(labels, np.int32, 0x7EADBEEF)
            self.byt = [lay(b, np.uint8, 0xEE) for b in self.byte_arrays]
            self.lengths = None
            self.off = off if off_override is None else np.array(off_override, dtype=np.uint64)

    def flags(self, keep_tail=False, mask_first=True):
        return (I64 if self.i64 else 0) | (PAD_LEFT if self.pad_left and self.form == "rows" else 0) | (KEEP_TAIL if keep_tail else 0) | \
            (MASK_FIRST if mask_first else 0)


OUT_NAMES = ("labels", "b0", "b1", "b2", "b3", "mask", "pos", "sid", "place", "fill", "cu", "n")


def out_arrays(n, R, L, i64):
    """every output of one call with a canary element behind it: name -> (array, canary value)"""
    dt = np.int64 if i64 else np.int32
    a = {"rows": np.full(R * L + 1, 0x5EADBEEF, dtype=dt), "labels": np.full(R * L + 1, 0x5A5A5A5A, dtype=dt),
         "mask": np.full(R * L + 1, 0x5A, dtype=np.uint8), "pos": np.full(R * L + 1, -9, dtype=np.int32),
         "sid": np.full(R * L + 1, -9, dtype=np.int32), "place": np.full(2 * n + 1, -9, dtype=np.int32),
         "fill": np.full(R + 1, -9, dtype=np.int32), "cu": np.full(n + R + 2, -1, dtype=np.int32), "n": np.full(5, -9, dtype=np.int64)}
    for k in range(4):
        a[f"b{k}"] = np.full(R * L + 1, 0x5A, dtype=np.uint8)
    return a


def to_packed(a, inp, n, R, L, status, null=()):
    """the arrays of out_arrays (canaries checked by the caller) as seqpack_ref.Packed: ids and labels int64"""
    get = lambda k: None if k in null else a[k][:-1]
    rows = a["rows"][:-1]
    ids = (rows if inp.i64 else rows.view(np.uint32)).astype(np.int64).reshape(R, L)
    lab = None if "labels" in null or inp.lab is None else a["labels"][:-1].astype(np.int64).reshape(R, L)
    byt = [None if f"b{k}" in null or inp.byt[k] is None else a[f"b{k}"][:-1].reshape(R, L) for k in range(4)]
    sh = lambda k: None if get(k) is None else get(k).reshape(R, L)
    return ref.Packed(ids, lab, byt, sh("mask"), sh("pos"), sh("sid"), None if "place" in null else a["place"][:-1].reshape(n, 2), get("fill"),
                      None if "cu" in null else a["cu"][:-1], get("n"), status)


def run(inp, L, strategy, *, max_rows=None, pad_id=0, ignore_index=-100, fills=(0, 0, 0, 0), keep_tail=False, mask_first=True,
        lds_max=None, null=()):
    """what the kernels' decisions give for one call -> seqpack_ref.Packed (outputs named in `null` were passed as NULL: None)"""
    n = inp.n
    R = n if max_rows is None else max_rows
    a = out_arrays(n, R, L, inp.i64)
    canary = {k: v[-1].copy() for k, v in a.items()}
    status = np.array([0, 0x5A5A5A5A], dtype=np.uint32)
    nb = work_bytes(n, R)
    work = np.full(nb // 8 + 1, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    ptr = lambda x: None if x is None else x.ctypes.data
    bin_ = (ctypes.c_void_p * 4)(*[ptr(b) for b in inp.byt])
    bout = (ctypes.c_void_p * 4)(*[None if f"b{k}" in null else a[f"b{k}"].ctypes.data for k in range(4)])
    out = lambda k: None if k in null else a[k].ctypes.data
    fl = fills[0] | fills[1] << 8 | fills[2] << 16 | fills[3] << 24
    rc = lib().sq_pack(ptr(inp.ids), ptr(inp.lengths), ptr(inp.off), ptr(inp.lab), bin_, n, inp.L_in, inp.flags(keep_tail, mask_first),
                       ref.STRATEGIES[strategy], L, pad_id, ignore_index & 0xFFFFFFFF, fl, R, geometry()["lds_max"] if lds_max is None else lds_max,
                       a["rows"].ctypes.data, out("labels"), bout, out("mask"), out("pos"), out("sid"), out("place"), out("fill"), out("cu"),
                       out("n"), status.ctypes.data, work.ctypes.data)
    assert rc == 0, "a restated LDS array was written past its end"
    assert all(a[k][-1] == canary[k] for k in a) and status[1] == 0x5A5A5A5A and work[-1] == 0x5A5A5A5A5A5A5A5A, "written past the end"
    for k in null:
        assert (a[k] == canary[k]).all(), f"{k} was passed as NULL and written"
    return to_packed(a, inp, n, R, L, int(status[0]), null)


def assert_equal(got, want, n_cu_from=None):
    """every output that `got` has equals the reference's; cu_seqlens over its n[2] entries"""
    assert (got.input_ids == want.input_ids).all()
    for g, w in [(got.labels, want.labels)] + list(zip(got.bytes, want.bytes)):
        if g is not None:
            assert w is not None and (g == w).all()
    for name in ("attention_mask", "position_ids", "seq_ids", "seq_place", "row_fill", "n"):
        g = getattr(got, name)
        if g is not None:
            assert (np.asarray(g) == np.asarray(getattr(want, name))).all(), name
    if got.cu_seqlens is not None:
        k = int(want.n[2])
        assert (got.cu_seqlens[:k] == want.cu_seqlens[:k]).all() and (got.cu_seqlens[k:len(want.cu_seqlens)] == -1).all()
    assert got.status == want.status


# ---------------------------------------------------------------------------------------------- the cases both test files walk
ROW_LENS = (1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 130)
N_SEQS = (0, 1, 2, 63, 64, 65, 130, 257)


def content(lengths, seed=1):
    """ids, labels and four byte arrays for sequences of these lengths: every value names its sequence and its position"""
    rng = np.random.default_rng(seed)
    seqs = [[(i * 1000 + j) % 100003 + 1 for j in range(l)] for i, l in enumerate(lengths)]
    labels = [[-100 if rng.integers(3) == 0 else v for v in s] for s in seqs]
    byts = tuple([[int((v * (k + 3)) % 251) for v in s] for s in seqs] for k in range(4))
    return seqs, labels, byts


def grid_cases():
    """(name, lengths, row_len): random lengths 0 .. row_len + 2 for every row_len x n_seqs of ROW_LENS x N_SEQS"""
    rng = np.random.default_rng(20)
    out = []
    for L in ROW_LENS:
        for n in N_SEQS:
            out.append((f"L{L}-n{n}", rng.integers(0, L + 3, size=n).tolist(), L))
    return out


def shaped_cases():
    """(name, lengths, row_len): lengths with a shape: all empty, all full, all too long, alternating, exact fills, equal runs, runs of empty sequences"""
    out = []
    for L in (1, 5, 8, 64):
        n = 70
        out += [(f"zeros-L{L}", [0] * n, L), (f"full-L{L}", [L] * n, L), (f"over-L{L}", [L + 1 + i % 3 for i in range(n)], L),
                (f"alt-L{L}", [1 if i % 2 == 0 else L for i in range(n)], L)]
    out += [("exact-fill", [3, 7, 4, 6, 5, 5, 10, 1, 9], 10), ("one-over", [3, 8, 4, 7, 5, 6, 10, 1, 10], 10),
            ("equal-runs", [4] * 9 + [3] * 11 + [4] * 5 + [2] * 13 + [3] * 7, 7), ("lifo", [4, 4, 3, 3, 3, 3], 7),
            ("lead-trail-empty", [0] * 70 + [5, 3, 0, 8, 2, 0, 0, 9] * 10 + [0] * 66, 9),
            ("many-small", [1] * 300, 130), ("one-long-many-small", [130] + [1] * 200 + [129], 130)]
    return out
