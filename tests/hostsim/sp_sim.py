"""ctypes wrapper of tests/hostsim/sp_sim.cpp (TEST TOOL; builds with g++, no GPU needed), and the texts the CPU and the GPU tests of
SentencePiece mode share."""
import ctypes
import os
import struct
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_CSRC = os.path.join(_ROOT, "splintr_amd", "csrc")
_LIB = os.path.join(_HERE, "libsp_sim.so")
sys.path.insert(0, os.path.dirname(_HERE))
import sp_ref  # noqa: E402

SPECIAL = {"<s>": 300, "</s>": 301}
# name -> documents of one batch.  Tile seams: the device tile is 4 096 bytes, the simulation's 64.
CASES = {
    "one_space": ["a b"],
    "spaces_before_word": ["a   ab", "ab  a"],
    "leading_trailing": ["  ab", "ab  ", " a "],
    "only_spaces": ["     ", " "],
    "space_newline_spaces": [" \n  x", "a \t\r\n b", "a\n\nb \n\n"],
    "not_ascii_led": ["\x0b x", "a\u00a0  b", "\u00a0 "],
    "multibyte_ws_as_bytes": [" \u3000x", "a \u2003\u00a0 b"],
    "literal_mark": ["a\u2581b \u2581", "\u2581\u2581 x"],
    "empty_between": ["", "a b", "", "", " c", ""],
    "run_across_documents": ["ab  ", "  ab", " ", " x"],
    "long_run": ["x" + " " * 9000 + "ab"],
    "word_over_seam": ["a " * 2040 + "ab" * 20 + " a", "z" * 60 + " " + "ab" * 5],
    "three_tiles": [("ab a  \n\tb  " * 1000)[:9001]],
    "seam_in_run": ["y" * 61 + "   ab", "y" * 62 + " \n  a", "y" * 60 + "     a" + " " * 70 + "b"],
    "specials": [" <s> a  </s>  b ", "<s></s> ", "a <s>"],
}


def build():
    src = os.path.join(_HERE, "sp_sim.cpp")
    deps = [src] + [os.path.join(_CSRC, f) for f in ("spl_k_sp.h", "spl_common.h")]
    if not os.path.exists(_LIB) or any(os.path.getmtime(d) > os.path.getmtime(_LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", _LIB, src])
    return _LIB


def class_table():
    """(stage1 uint16, stage2 uint8, shift) of splintr_amd/data/unicode_classes.bin, as spl_tables.cpp reads them."""
    with open(os.path.join(_ROOT, "splintr_amd", "data", "unicode_classes.bin"), "rb") as f:
        blob = f.read()
    shift, nblocks = struct.unpack_from("<II", blob, 8)
    n1 = 0x110000 >> shift
    return (np.frombuffer(blob, dtype=np.uint16, count=n1, offset=32).copy(),
            np.frombuffer(blob, dtype=np.uint8, count=nblocks << shift, offset=32 + 2 * n1).copy(), shift)


def scan_bitmaps(texts, special):
    """What k_mark_docs / k_special_scan leave over the packed texts: text starts (documents, and behind every literal), tokens
    (a literal's first byte), literal bytes."""
    n = sum(len(t.encode()) for t in texts)
    bm = np.zeros((3, n // 32 + 2), dtype=np.uint32)
    pos = 0
    for t in texts:
        if pos < n:
            bm[0, pos >> 5] |= np.uint32(1 << (pos & 31))
        for item in sp_ref.split_special(t, special):
            ln = len((item[1] if item[0] == "text" else item[2]).encode())
            if item[0] == "special":
                bm[1, pos >> 5] |= np.uint32(1 << (pos & 31))
                for q in range(pos, pos + ln):
                    bm[2, q >> 5] |= np.uint32(1 << (q & 31))
                if pos + ln < n:
                    bm[0, (pos + ln) >> 5] |= np.uint32(1 << ((pos + ln) & 31))
            pos += ln
    return bm


def rewrite(texts, tile=64, special=None):
    """-> (rewritten bytes, sorted chunk starts, rewritten document offsets) from the shared tile logic."""
    L = ctypes.CDLL(build())
    L.sp_sim_rewrite.restype = ctypes.c_uint64
    L.sp_sim_rewrite.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                                 ctypes.c_uint32] + [ctypes.c_void_p] * 3 + [ctypes.c_uint32] + [ctypes.c_void_p] * 3
    parts = [t.encode() for t in texts]
    text = np.frombuffer(b"".join(parts) + b"\0" * 16, dtype=np.uint8).copy()
    n = len(text) - 16
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    np.cumsum([len(p) for p in parts], out=off[1:])
    s1, s2, shift = class_table()
    bm = scan_bitmaps(texts, special) if special else None
    out = np.zeros(3 * n + 16, dtype=np.uint8)
    bits = np.zeros(3 * n // 32 + 2, dtype=np.uint32)
    ooff = np.zeros(len(parts) + 1, dtype=np.uint64)
    p = lambda a: a.ctypes.data
    n_out = L.sp_sim_rewrite(p(text), n, p(off), len(parts), p(s1), p(s2), shift, *([p(bm[0]), p(bm[1]), p(bm[2])] if special else [None] * 3),
                             tile, p(out), p(bits), p(ooff))
    starts = [i for i in range(n_out) if (int(bits[i >> 5]) >> (i & 31)) & 1]
    return out[:n_out].tobytes(), starts, ooff.tolist()
