"""ctypes wrapper of tests/hostsim/chat_sim.cpp (TEST TOOL; builds with g++, no GPU needed)."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "splintr_amd", "csrc")
_LIB = os.path.join(_HERE, "libchat_sim.so")

OUTPUTS = ("labels", "loss", "mask", "role", "special", "len", "kept", "turn_col")


def build():
    src = os.path.join(_HERE, "chat_sim.cpp")
    deps = [src] + [os.path.join(_CSRC, f) for f in ("spl_k_chat.h", "spl_k_pair.h", "spl_k_collate.h", "spl_k_seqscan.h", "spl_common.h")]
    if not os.path.exists(_LIB) or any(os.path.getmtime(d) > os.path.getmtime(_LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", _LIB, src])
    return _LIB


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(build())
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        src = [vp, vp, u32, vp, vp, vp, u32, vp, u32, u32, u32, u32, u32, u32, u32, u32, vp, vp, vp, vp, vp, u32, vp, u32]
        L.cs_geometry.argtypes = [vp]
        L.cs_work_bytes.argtypes = [u64, u64]
        L.cs_work_bytes.restype = u64
        L.cs_chat.argtypes = src + [vp] * 11
        L.cs_groups.argtypes = src + [vp, u32] + [vp] * 8
        _lib = L
    return _lib


def geometry():
    g = np.zeros(5, dtype=np.uint32)
    lib().cs_geometry(g.ctypes.data)
    return dict(zip(["lanes", "vec", "span", "waves", "rec_bytes"], g.tolist()))


def work_bytes(n_turns, n_convs):
    return int(lib().cs_work_bytes(n_turns, n_convs))


def _src_args(case, pad_id, ignore_id):
    """case: chat_ref.Case (ids, off, n_docs, turn_doc, turn_role, turn_train, n_turns, conv_off, n_convs, L, flags, tpl)"""
    tpl = case.tpl
    n_roles = len(tpl.roles)
    n_header = np.zeros(8, dtype=np.uint32)
    n_footer = np.zeros(8, dtype=np.uint32)
    header = np.zeros((8, 16), dtype=np.uint32)
    footer = np.zeros((8, 8), dtype=np.uint32)
    for r, (h, f) in enumerate(tpl.roles):
        n_header[r], n_footer[r] = len(h), len(f)
        header[r, :len(h)] = h
        footer[r, :len(f)] = f
    opt = lambda a, dt: None if a is None else np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=dt), np.zeros(1, dtype=dt)]))
    keep = [opt(case.ids, np.uint32), np.ascontiguousarray(case.off, dtype=np.uint64), opt(case.turn_doc, np.int32),
            opt(case.turn_role, np.uint8), opt(case.turn_train, np.uint8), np.ascontiguousarray(case.conv_off, dtype=np.uint64),
            n_header, n_footer, header, footer, np.array(list(tpl.bos) + [0], dtype=np.uint32), np.array(list(tpl.gen) + [0], dtype=np.uint32)]
    ptr = lambda a: None if a is None else a.ctypes.data
    args = [ptr(keep[0]), ptr(keep[1]), case.n_docs, ptr(keep[2]), ptr(keep[3]), ptr(keep[4]), case.n_turns, ptr(keep[5]), case.n_convs,
            case.flags & ~1, case.L, pad_id, ignore_id, n_roles, tpl.train_content, tpl.train_footer, ptr(n_header), ptr(n_footer), ptr(header),
            ptr(footer), ptr(keep[10]), len(tpl.bos), ptr(keep[11]), len(tpl.gen)]
    return args, keep


def _work(n_turns, n_convs):
    nb = work_bytes(n_turns, n_convs)
    w = np.full(nb // 8 + 1, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    return w


def chat(case, pad_id, ignore_id, null=(), unwritten=-7):
    """-> dict of rows uint32 [n_convs, L], labels int64, loss / mask / role / special uint8, len int32, kept int32 [n_convs, 2], turn_col
    int32 [n_turns, 2] (pre-filled with `unwritten`), status: what the kernels' mapping gives.  Every array has one canary element behind
    it.  null: names of optional outputs passed as NULL (they come back None)."""
    args, keep = _src_args(case, pad_id, ignore_id)
    n, L, nt = case.n_convs, case.L, case.n_turns
    a = {"rows": np.full(n * L + 1, 0xDEADBEEF, dtype=np.uint32), "labels": np.full(n * L + 1, 0x5A5A5A5A5A5A5A5A, dtype=np.int64),
         "len": np.full(n + 1, -9, dtype=np.int32), "kept": np.full(2 * n + 1, -9, dtype=np.int32),
         "turn_col": np.full(2 * nt + 1, unwritten, dtype=np.int32)}
    for name in ("loss", "mask", "role", "special"):
        a[name] = np.full(n * L + 1, 0x5A, dtype=np.uint8)
    canary = {k: v[-1].copy() for k, v in a.items()}
    status = np.array([0, 0x5A5A5A5A], dtype=np.uint32)
    work = _work(nt, n)
    ptr = lambda name: None if name in null else a[name].ctypes.data
    assert lib().cs_chat(*args, a["rows"].ctypes.data, ptr("labels"), ptr("loss"), ptr("mask"), ptr("role"), ptr("special"), ptr("len"),
                         ptr("kept"), ptr("turn_col"), status.ctypes.data, work.ctypes.data) == 0
    assert all(a[k][-1] == canary[k] for k in a) and status[1] == 0x5A5A5A5A and work[-1] == 0x5A5A5A5A5A5A5A5A, "written past the end"
    out = {}
    for name, arr in a.items():
        if name in null:
            assert (arr == canary[name]).all(), f"{name} was passed as NULL and written"
            out[name] = None
        else:
            out[name] = arr[:-1] if name == "len" else arr[:-1].reshape(-1, 2) if name in ("kept", "turn_col") else arr[:-1].reshape(n, L)
    out["status"] = int(status[0])
    return out


def groups(case, pad_id, ignore_id, e0):
    """The turns, then the groups of four elements that start at the flat indices e0 (multiples of 4), for outputs that no memory holds:
    -> values uint32 [len(e0), 4], bits / roles uint8 [len(e0), 4] (bits: 1 mask, 2 loss, 4 special), len, kept, turn_col, status"""
    args, keep = _src_args(case, pad_id, ignore_id)
    e0 = np.ascontiguousarray(e0, dtype=np.uint64)
    k, n, nt = len(e0), case.n_convs, case.n_turns
    v = np.full(4 * k + 1, 0xDEADBEEF, dtype=np.uint32)
    bits, roles = (np.full(k + 1, 0x5A5A5A5A, dtype=np.uint32) for _ in range(2))
    lens, kept, tc = np.full(n + 1, -9, dtype=np.int32), np.full(2 * n + 1, -9, dtype=np.int32), np.full(2 * nt + 1, -7, dtype=np.int32)
    status = np.array([0, 0x5A5A5A5A], dtype=np.uint32)
    work = _work(nt, n)
    assert lib().cs_groups(*args, e0.ctypes.data, k, v.ctypes.data, bits.ctypes.data, roles.ctypes.data, lens.ctypes.data, kept.ctypes.data,
                           tc.ctypes.data, status.ctypes.data, work.ctypes.data) == 0
    assert v[-1] == 0xDEADBEEF and bits[-1] == roles[-1] == 0x5A5A5A5A and lens[-1] == -9 and kept[-1] == -9 and tc[-1] == -7 and \
        status[1] == 0x5A5A5A5A and work[-1] == 0x5A5A5A5A5A5A5A5A
    by = lambda a: a[:-1].copy().view(np.uint8).reshape(k, 4)              # (little endian: byte i is element i)
    return v[:-1].reshape(k, 4), by(bits), by(roles), lens[:-1], kept[:-1].reshape(n, 2), tc[:-1].reshape(nt, 2), int(status[0])
