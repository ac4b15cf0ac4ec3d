"""Reader and writer of the code-point class table (splintr_amd/data/unicode_classes*.bin; the format is stated in
tools/gen_unicode_tables.py) for tests: a shipped table read into flat arrays, edited, and written back as a valid file
with both two-stage tables rebuilt.  Plain Python + numpy, no GPU."""
import os
import struct
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np

DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "splintr_amd", "data")
CLASS_NAMES = ["P", "AP", "SP", "WS", "NL", "N", "Lu", "Ll", "Lt", "Lm", "Lo", "M"]
GC_NAMES = ["Cn", "Lu", "Ll", "Lt", "Lm", "Lo", "Mn", "Mc", "Me", "Nd", "Nl", "No", "Pc", "Pd", "Ps", "Pe", "Pi", "Pf", "Po",
            "Sm", "Sc", "Sk", "So", "Zs", "Zl", "Zp", "Cc", "Cf", "Cs", "Co"]
N_CP = 0x110000


@dataclass
class Table:
    version: int
    shift: int
    unicode_version: bytes                      # the header's 16-byte field, as stored
    cls: np.ndarray                             # uint8[0x110000], index into CLASS_NAMES
    folds: List[Tuple[int, int]]                # (code point, ascii lower-case letter)
    gc: np.ndarray = None                       # uint8[0x110000], index into GC_NAMES (version >= 2)
    scripts: List[Tuple[str, List[Tuple[int, int]]]] = field(default_factory=list)     # (name, inclusive ranges) (version 3)

    @property
    def engine_version(self) -> str:
        return self.unicode_version.rstrip(b"\0").decode()


def _flat(blob: bytes, at: int, shift: int, n_blocks: int):
    """one two-stage table at `at` -> (flat uint8[0x110000], offset behind it)"""
    n1 = N_CP >> shift
    s1 = np.frombuffer(blob, dtype="<u2", count=n1, offset=at).astype(np.int64)
    assert int(s1.max()) < n_blocks, "block index out of range"
    s2 = np.frombuffer(blob, dtype=np.uint8, count=n_blocks << shift, offset=at + 2 * n1)
    cp = np.arange(N_CP, dtype=np.int64)
    return s2[(s1[cp >> shift] << shift) | (cp & ((1 << shift) - 1))].copy(), at + 2 * n1 + (n_blocks << shift)


def read_table(path: str) -> Table:
    if not os.path.isabs(path):
        path = os.path.join(DATA, path)
    with open(path, "rb") as f:
        blob = f.read()
    magic, version, shift, n_blocks, uver = struct.unpack_from("<4sIII16s", blob, 0)
    assert magic == b"SPLU" and 1 <= version <= 3, (magic, version)
    cls, at = _flat(blob, 32, shift, n_blocks)
    (n_fold,) = struct.unpack_from("<I", blob, at)
    folds = [struct.unpack_from("<II", blob, at + 4 + 8 * i) for i in range(n_fold)]
    at += 4 + 8 * n_fold
    t = Table(version, shift, uver, cls, folds)
    if version >= 2:
        (gnb,) = struct.unpack_from("<I", blob, at)
        t.gc, at = _flat(blob, at + 4, shift, gnb)
    if version >= 3:
        (ns,) = struct.unpack_from("<I", blob, at)
        at += 4
        for _ in range(ns):
            name, nr = struct.unpack_from("<32sI", blob, at)
            at += 36
            rs = [struct.unpack_from("<II", blob, at + 8 * q) for q in range(nr)]
            at += 8 * nr
            t.scripts.append((name.rstrip(b"\0").decode(), rs))
    assert at == len(blob), (at, len(blob))                 # nothing behind the last section: the file is not truncated or padded
    return t


def _two_stage(flat: np.ndarray, shift: int):
    """blocks numbered in order of first appearance, as tools/gen_unicode_tables.py numbers them"""
    bs = 1 << shift
    blocks: Dict[bytes, int] = {}
    stage1, stage2 = [], bytearray()
    raw = flat.tobytes()
    for b in range(N_CP >> shift):
        blk = raw[b * bs:(b + 1) * bs]
        idx = blocks.get(blk)
        if idx is None:
            idx = blocks[blk] = len(blocks)
            stage2 += blk
        stage1.append(idx)
    return stage1, bytes(stage2), len(blocks)


def table_bytes(t: Table) -> bytes:
    s1, s2, nb = _two_stage(t.cls, t.shift)
    out = bytearray(struct.pack("<4sIII16s", b"SPLU", t.version, t.shift, nb, t.unicode_version))
    out += struct.pack(f"<{len(s1)}H", *s1) + s2
    out += struct.pack("<I", len(t.folds))
    for cp, lo in t.folds:
        out += struct.pack("<II", cp, lo)
    if t.version >= 2:
        g1, g2, gnb = _two_stage(t.gc, t.shift)
        out += struct.pack("<I", gnb) + struct.pack(f"<{len(g1)}H", *g1) + g2
    if t.version >= 3:
        out += struct.pack("<I", len(t.scripts))
        for name, rs in t.scripts:
            out += struct.pack("<32sI", name.encode(), len(rs))
            for a, b in rs:
                out += struct.pack("<II", a, b)
    return bytes(out)


def write_edited(src: str, dst: str, class_edits: Dict[int, str]) -> Table:
    """`src` with the class of the given code points replaced (names of CLASS_NAMES), written to `dst`; header version untouched."""
    t = read_table(src)
    for cp, name in class_edits.items():
        t.cls[cp] = CLASS_NAMES.index(name)
    with open(dst, "wb") as f:
        f.write(table_bytes(t))
    return t


# U+4E00..U+9FFF and U+AC00..U+D7A3 are what the kernels' CJK short cut answers without a table look-up when the whole of
# both ranges is Lo.  With the first and the last code point of each range made a number the short cut must be off, and the
# code points next to the ranges keep what the table says.
CJK_EDGE_EDITS = {0x4E00: "N", 0x9FFF: "N", 0xAC00: "N", 0xD7A3: "N"}
CJK_EDGE_KEPT = (0x4DFF, 0xA000, 0xABFF, 0xD7A4)
