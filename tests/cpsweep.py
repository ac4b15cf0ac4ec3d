"""Every Unicode scalar value, in contexts, as documents for the scanner and the splitter (plain Python + numpy, no GPU).

A document is one CONTEXT -- a short template in which X stands for the code point -- repeated over a block of consecutive
code points: block U+0041.. in context 'aX ' is b"aA aB aC ...".  Documents may begin with a few '.' so that, in the packed
batch (the concatenation the tokenizer receives), a code point's first byte falls on a chosen offset modulo 4: the tile
kernel classifies text four bytes to a word, and a character that starts at byte 1, 2 or 3 of a word, or whose lead byte
lies in the word before, takes other code than one at byte 0.

full_sweep()     every code point in all FULL_CONTEXTS, at all four byte offsets mod 4, and once as a document of its own
                 (first and last character of a document).  A range that the class table proves uniform (one class, one
                 general category: the unassigned planes) goes through THIN_CONTEXT only, at rotating alignment.
reduced_sweep()  every code point once, in REDUCED_CONTEXT, alignment rotated per block.

Both verify what they promise before they return (Sweep.check_*), and Sweep.describe turns a byte of a document back into
"U+XXXX in context 'aX '"."""
from typing import List, Optional, Sequence, Tuple

import numpy as np

from uclassgen import read_table

SCANNER_CONTEXTS = ["aX ", " Xa\n", "1X'sX", "XX\n", " X1", ".X", "AXb"]
# the contraction letters with X in the letter's place and behind it (the fold list: U+017F is an s under (?i)), the four of one
# period b'lX b'Xl c'rX c'vX also being what guarantees the four alignments of a block of characters of one length
CONTRACTION_CONTEXTS = ["a'X ", "b'lX ", "b'Xl ", "c'rX ", "c'vX "]
MARK_CONTEXT = "a\u0301X"
FULL_CONTEXTS = SCANNER_CONTEXTS + CONTRACTION_CONTEXTS + [MARK_CONTEXT]
REDUCED_CONTEXT = "aX 1X\n"
THIN_CONTEXT = "X "
SOLO_CONTEXT = "X"
ALL_RANGES = ((0, 0x10FFFF),)
# U+40000..U+DFFFF: planes 4 to 13, unassigned in every Unicode version so far.  (Plane 3 is NOT uniform: U+30000..U+3134A are
# Lo in Unicode 14 already, so it goes through all contexts.)  uniform_range() proves the claim from the table file.
THIN_RANGE = (0x40000, 0xDFFFF)
PAD = b"."


def scalar_values(ranges) -> np.ndarray:
    """code points of inclusive (first, last) ranges, or of any iterable of code points, in order, without surrogates"""
    ranges = list(ranges)
    if ranges and isinstance(ranges[0], (tuple, list)):
        cps = np.concatenate([np.arange(a, b + 1, dtype=np.int64) for a, b in ranges])
    else:
        cps = np.asarray(ranges, dtype=np.int64)
    return cps[(cps < 0xD800) | (cps > 0xDFFF)]


def utf8_len(cps: np.ndarray) -> np.ndarray:
    return 1 + (cps >= 0x80) + (cps >= 0x800) + (cps >= 0x10000)


def uniform_range(table_file: str = "unicode_classes.bin", rng: Tuple[int, int] = THIN_RANGE) -> Tuple[int, int]:
    """(class, general category) of EVERY code point of `rng` in the table file; AssertionError if there is more than one of either"""
    t = read_table(table_file)
    a, b = rng
    cls, gc = np.unique(t.cls[a:b + 1]), np.unique(t.gc[a:b + 1])
    assert len(cls) == 1 and len(gc) == 1, f"U+{a:04X}..U+{b:04X} is not uniform in {table_file}: classes {cls.tolist()}, categories {gc.tolist()}"
    return int(cls[0]), int(gc[0])


class Sweep:
    def __init__(self):
        self.docs: List[bytes] = []
        self.contexts: List[str] = []
        self._cps: List[np.ndarray] = []          # one array per context section
        self._meta: List[Tuple[int, int, int, int]] = []     # per document: section, first and last+1 index into the section's code points, pad
        self._n_bytes = 0
        self._align = np.zeros(0x110000, dtype=np.int64)      # per code point: bit mask of (first byte's offset in the packed batch) & 3
        self._first = set()
        self._last = set()

    # ------------------------------------------------------------------ building
    def add(self, context: str, cps: np.ndarray, block: int, rotate: int = 0, padded: bool = True):
        """one section: `cps` in blocks of `block` per document; a document's first X is put at offset (block index + rotate) & 3
        of the packed batch by leading pad bytes (`padded`), or the documents are left as they are"""
        assert "X" in context and len(cps)
        sec = len(self.contexts)
        self.contexts.append(context)
        self._cps.append(cps)
        tpl = np.array([ord(c) for c in context], dtype=np.int64)
        xcol = np.nonzero(tpl == ord("X"))[0]
        arr = np.tile(tpl, (len(cps), 1))
        arr[:, xcol] = cps[:, None]
        blob = arr.astype("<u4").tobytes().decode("utf-32-le").encode("utf-8")
        ulen = utf8_len(cps)
        fixed = sum(len(c.encode("utf-8")) for c in context if c != "X")
        plen = fixed + len(xcol) * ulen                          # bytes per piece
        pstart = np.concatenate([[0], np.cumsum(plen)])
        # offset of every X inside its piece: the template's bytes before it, earlier X's counted with this code point's length
        before = [sum(len(c.encode("utf-8")) for c in context[:j] if c != "X") for j in xcol]
        xoff = np.stack([before[i] + i * ulen for i in range(len(xcol))], axis=1)       # (n, X's per piece)
        first = np.arange(0, len(cps), block)
        last = np.minimum(first + block, len(cps))
        blen = (pstart[last] - pstart[first]).tolist()
        x0 = xoff[first, 0].tolist()
        pads, at = [], self._n_bytes                             # (the only sequential part: a pad depends on all lengths before it)
        doc_at = []
        for bi, n in enumerate(blen):
            pad = (bi + rotate - at - x0[bi]) & 3 if padded else 0
            pads.append(pad)
            doc_at.append(at + pad)
            at += pad + n
        self._n_bytes = at
        lo, hi = pstart[first].tolist(), pstart[last].tolist()
        self.docs.extend(PAD * pad + blob[a:b] for pad, a, b in zip(pads, lo, hi))
        self._meta.extend((sec, a, b, pad) for a, b, pad in zip(first.tolist(), last.tolist(), pads))
        # where every X of every piece starts in the packed batch
        base = np.repeat(np.asarray(doc_at, dtype=np.int64) - pstart[first], last - first)
        masks = np.bitwise_or.reduce(1 << ((base[:, None] + pstart[:-1, None] + xoff) & 3), axis=1)
        if xcol[0] == 0:
            self._first.update(cps[first[np.asarray(pads) == 0]].tolist())
        if xcol[-1] == len(tpl) - 1:
            self._last.update(cps[last - 1].tolist())
        np.bitwise_or.at(self._align, cps, masks)

    def add_at(self, context: str, cp: int, align: int):
        """one document of one piece whose first X starts at `align` mod 4 (what a block of mixed lengths left open)"""
        self.add(context, np.array([cp], dtype=np.int64), 1, rotate=align)

    # ------------------------------------------------------------------ reading
    @property
    def n_bytes(self) -> int:
        return self._n_bytes

    def packed(self):
        """(uint8 text, uint64 offsets[N+1]) of the batch"""
        off = np.zeros(len(self.docs) + 1, dtype=np.uint64)
        np.cumsum([len(d) for d in self.docs], out=off[1:])
        return np.frombuffer(b"".join(self.docs), dtype=np.uint8), off

    def texts(self) -> List[str]:
        return [d.decode("utf-8") for d in self.docs]

    def locate(self, doc: int, byte: int) -> Tuple[Optional[int], str]:
        """(code point of the piece byte `byte` of document `doc` lies in -- None inside the leading pad --, context)"""
        sec, a, b, pad = self._meta[doc]
        ctx, cps = self.contexts[sec], self._cps[sec][a:b]
        fixed = sum(len(c.encode("utf-8")) for c in ctx if c != "X")
        ends = pad + np.cumsum(fixed + ctx.count("X") * utf8_len(cps))
        if byte < pad:
            return None, ctx
        k = min(int(np.searchsorted(ends, byte, side="right")), len(cps) - 1)
        return int(cps[k]), ctx

    def describe(self, doc: int, byte: int) -> str:
        cp, ctx = self.locate(doc, byte)
        sec, a, b, _ = self._meta[doc]
        where = "the leading pad" if cp is None else f"U+{cp:04X}"
        return f"{where} in context {ctx!r} (document {doc}: U+{int(self._cps[sec][a]):04X}..U+{int(self._cps[sec][b - 1]):04X}, byte {byte})"

    def code_points(self, doc: int) -> np.ndarray:
        sec, a, b, _ = self._meta[doc]
        return self._cps[sec][a:b]

    # ------------------------------------------------------------------ what the sweep promises
    def alignments_missing(self, cps: np.ndarray) -> List[Tuple[int, int]]:
        short = cps[self._align[cps] != 15]
        return [(cp, k) for cp in short.tolist() for k in range(4) if not int(self._align[cp]) >> k & 1]

    def check_alignments(self, cps: np.ndarray, every: bool = True):
        if every:
            miss = self.alignments_missing(cps)
            assert not miss, f"{len(miss)} (code point, offset mod 4) pairs never occur, first U+{miss[0][0]:04X} at {miss[0][1]}"
        else:
            miss = cps[self._align[cps] == 0]
            assert not len(miss), f"{len(miss)} code points never occur, first U+{int(miss[0]):04X}"

    def check_first_and_last(self, cps: np.ndarray):
        want = set(cps.tolist())
        assert want <= self._first, f"{len(want - self._first)} code points never begin a document, e.g. U+{min(want - self._first):04X}"
        assert want <= self._last, f"{len(want - self._last)} code points never end a document, e.g. U+{min(want - self._last):04X}"


def sweep_docs(contexts: Sequence[str], block: int = 64, ranges=ALL_RANGES, solo: bool = False, thin=None) -> Sweep:
    """`ranges` through every context of `contexts` in documents of `block` code points; all four alignments of every code point
    are asserted when there are at least four contexts (documents of one piece are added for what the blocks left open), one
    otherwise.  `thin`: a (first, last) range that only goes through THIN_CONTEXT (the caller has shown it uniform).  `solo`:
    also every code point as a document of its own."""
    cps = scalar_values(ranges)
    dense = cps if thin is None else cps[(cps < thin[0]) | (cps > thin[1])]
    sparse = cps[:0] if thin is None else cps[(cps >= thin[0]) & (cps <= thin[1])]
    s = Sweep()
    for ci, ctx in enumerate(contexts):
        s.add(ctx, dense, block, rotate=ci)
    if len(sparse):
        s.add(THIN_CONTEXT, sparse, block)
    every = len(contexts) >= 4
    if every:
        for cp, k in s.alignments_missing(dense):
            s.add_at(contexts[0], cp, k)
    if solo:
        s.add(SOLO_CONTEXT, cps, 1, padded=False)
        s.check_first_and_last(cps)
    s.check_alignments(dense, every)
    s.check_alignments(sparse, False)
    return s


_cache = {}


def full_sweep(ranges=ALL_RANGES, table_file: str = "unicode_classes.bin") -> Sweep:
    """all contexts, four alignments, every code point also alone; THIN_RANGE thinned after the table file has shown it uniform.
    Cached: callers must not change what they get."""
    key = ("full", tuple(map(tuple, ranges)) if isinstance(ranges[0], (tuple, list)) else tuple(ranges), table_file)
    if key not in _cache:
        uniform_range(table_file, THIN_RANGE)
        _cache[key] = sweep_docs(FULL_CONTEXTS, 64, ranges, solo=True, thin=THIN_RANGE)
    return _cache[key]


def full_contexts(ranges) -> Sweep:
    """all contexts and four alignments over a few ranges or a list of code points (nothing thinned, no documents of one character)"""
    return sweep_docs(FULL_CONTEXTS, 64, ranges)


def reduced_sweep() -> Sweep:
    if "reduced" not in _cache:
        s = sweep_docs([REDUCED_CONTEXT], 64, ALL_RANGES)
        seen = np.concatenate([s.code_points(d) for d in range(len(s.docs))])
        assert len(seen) == 1112064 and np.array_equal(seen, scalar_values(ALL_RANGES))      # every scalar value, once
        _cache["reduced"] = s
    return _cache["reduced"]


def first_difference(sweep: Sweep, got, want, token_bytes, first_doc: int = 0) -> str:
    """Where two CSR results (ids, offsets) over the sweep's documents from `first_doc` on first differ, as a code point in a
    context.  `token_bytes(ids)` gives the bytes a list of ids stands for (the prefix both sides agree on locates the byte)."""
    g_ids, g_off = got
    w_ids, w_off = want
    if len(g_off) != len(w_off):
        return f"{len(g_off) - 1} documents instead of {len(w_off) - 1}"
    same = (g_off[1:] - g_off[:-1]) == (w_off[1:] - w_off[:-1])
    n = min(len(g_ids), len(w_ids))
    neq = np.nonzero(g_ids[:n] != w_ids[:n])[0]
    cands = [int(np.nonzero(~same)[0][0])] if not same.all() else []
    if len(neq):
        cands.append(int(np.searchsorted(w_off, int(neq[0]), side="right")) - 1)
    if not cands:
        return "no document differs (the totals do)"
    d = min(cands)
    g, w = g_ids[int(g_off[d]):int(g_off[d + 1])], w_ids[int(w_off[d]):int(w_off[d + 1])]
    k = next((i for i, (x, y) in enumerate(zip(g.tolist(), w.tolist())) if x != y), min(len(g), len(w)))
    doc = sweep.docs[first_doc + d]
    byte = len(token_bytes(w[:k].tolist()))
    return (f"{sweep.describe(first_doc + d, min(byte, len(doc) - 1))}: ids {g[k:k + 6].tolist()} instead of {w[k:k + 6].tolist()} "
            f"for {doc[byte:byte + 12]!r}")


# ------------------------------------------------------------------------------------------------
# worker of the CPU comparison "C oracle == PCRE2" (a process pool: the PCRE2 side is a Python loop per match)
# ------------------------------------------------------------------------------------------------
def split_check_worker(task):
    """(first document index, documents, pattern names) -> per name (first differing document or -1, seconds PCRE2, seconds oracle)"""
    import time
    from oracle import pyoracle as O
    from oracle.coracle import COracle
    first, docs, names = task
    out = {}
    for name in names:
        rx, c = O.Pcre2Pattern(O.PRETRAINED[name][1]), COracle(name)
        t0 = time.perf_counter()
        want = [[a for a, _ in rx.find_iter(d)] for d in docs]
        t1 = time.perf_counter()
        got = [c.split_bytes(d) for d in docs]
        t2 = time.perf_counter()
        bad = next((i for i, (g, w) in enumerate(zip(got, want)) if g != w), -1)
        out[name] = (first + bad if bad >= 0 else -1, t1 - t0, t2 - t1)
    return out
