"""GPU tests (-m gpu) of a warm tile's way through k_pretok (csrc/spl_k_pretok.h), every result compared with the oracle:

  the merge phase         -- a tile without a miss leaves it at once (no sort, no pull, no closing barrier), a tile with only medium misses
     skips the sort: batches in which no tile, only the middle tile, or every tile has misses, memo on (cold, filling, warm) and off,
     as one launch and as two (the form asserted from the profile, as tests/test_gpu_fused.py does).
  two-byte text           -- what the classify phase makes of the characters C2's text beyond ASCII consists of (csrc/spl_scan_words.h):
     two-byte and General Punctuation characters at every byte alignment, across the tile boundary, at the first and last bytes of a
     document and of the corpus, the code points U+07FF / U+0800 / U+1FFF / U+2000 / U+207F / U+2080, overlong and truncated forms;
     three split patterns, both Unicode tables.  These cases run code this file's commit did not change: the classifier as it was.  They
     were written for a class table of these code points in LDS, which measured as no gain and is not in the code
     (profiles/warm_tile_path.txt, "B"); they stay as the parity cases any such short cut has to keep.

Every batch is three tiles of 800 bytes."""
import os

import numpy as np
import pytest

from test_gpu_fused import _dev, _encode, _opt, _profile, _same

pytestmark = pytest.mark.gpu

TILE = 800
UCLS = {"pcre2": "unicode_classes.bin", "regex": "unicode_classes_regex.bin"}


# ------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------
_oracles = {}


def _oracle(name, tables="pcre2"):
    """The C oracle of `name` on either Unicode table (oracle.coracle.COracle reads the default one)."""
    from oracle import coracle as C
    if (name, tables) not in _oracles:
        if tables == "pcre2":
            _oracles[(name, tables)] = C.COracle(name)
        else:
            class _Other(C.COracle):
                def __init__(self, name):
                    fn, pid, bl, _ = C._REG[name]
                    self.name = name
                    self._h = C.lib().orc_create(os.path.join(C._DATA, fn).encode(), os.path.join(C._DATA, UCLS[tables]).encode(), pid, bl)
                    if not self._h:
                        raise IOError("orc_create failed")
            _oracles[(name, tables)] = _Other(name)
    return _oracles[(name, tables)]


def _raw_batch(docs):
    """A DeviceBatch of raw byte strings (DeviceBatch itself takes str: no way to pass text that is not UTF-8)."""
    import torch
    from splintr_amd.device import DeviceBatch
    b = DeviceBatch.__new__(DeviceBatch)
    buf = b"".join(docs)
    off = np.zeros(len(docs) + 1, dtype=np.uint64)
    np.cumsum([len(d) for d in docs], out=off[1:])
    b.n_docs, b.n_bytes = len(docs), len(buf)
    host = np.frombuffer(buf + b"\0" * ((-len(buf)) % 16 + 16), dtype=np.uint8)
    b.text = torch.from_numpy(host.copy()).to(_dev())
    b.doc_off = torch.from_numpy(off.astype(np.int64)).to(_dev())
    b.ids = torch.empty(max(b.n_bytes, 1), dtype=torch.int32, device=_dev())
    b.out_off = torch.zeros(b.n_docs + 1, dtype=torch.int64, device=_dev())
    b.host_offsets = off
    return b


def _want(orc, docs):
    off = np.zeros(len(docs) + 1, dtype=np.uint64)
    np.cumsum([len(d) for d in docs], out=off[1:])
    return orc.encode_packed(np.frombuffer(b"".join(docs), dtype=np.uint8), off, threads=8)


def enc(cp):
    if cp < 0x80:
        return bytes([cp])
    if cp < 0x800:
        return bytes([0xC0 | cp >> 6, 0x80 | cp & 0x3F])
    return bytes([0xE0 | cp >> 12, 0x80 | (cp >> 6) & 0x3F, 0x80 | cp & 0x3F])


E, DASH, QUOTE = enc(0xE9), enc(0x2014), enc(0x2019)


# ------------------------------------------------------------------------------------------------
# two-byte text and General Punctuation
# ------------------------------------------------------------------------------------------------
def _two_byte_docs(at_edge):
    """Documents of about three tiles; `at_edge` is the character whose first byte is corpus byte 799 (the tile boundary is 799 | 800)."""
    docs = [
        E + b"cole na" + enc(0xEF) + b"ve caf" + E + b" r" + E + b"sum" + E + b" Z" + enc(0xFC) + b"rich S" + enc(0xE3) + b"o " + DASH,     # first and last bytes of the corpus' first document
        DASH + b" it" + QUOTE + b"s " + enc(0x201C) + b"quoted" + enc(0x201D) + b" " + enc(0x2013) + b" and on" + enc(0x2026) + E,
        # the last two-byte code point, the first three-byte one, the edges of General Punctuation: next to ASCII and next to each other
        b"a" + enc(0x7FF) + b"b" + enc(0x800) + b"c" + enc(0x1FFF) + b"d" + enc(0x2000) + b"e" + enc(0x207F) + b"f" + enc(0x2080) + b"g " +
        enc(0x7FF) + enc(0x800) + enc(0x1FFF) + enc(0x2000) + enc(0x207F) + enc(0x2080) + enc(0x7FF) + b" h",
        # overlong forms, a lead without its continuation, a stray continuation byte
        b"o\xC0\x80v \xC1\xBFer \xE0\x80\x80long \xE0\x9F\xBF x\xC3y \xE2\x80z w\x80v \xA9 " + E + b"\xA9 \xC3" + E + b" end\xC3",
        b"\xA9starts inside a character, ends inside one \xE2\x80",
        b"\x94 " + enc(0x3B1) + enc(0x3B2) + enc(0x3B3) + b" " + enc(0x416) + enc(0x438) + b" " + enc(0x5D0) + enc(0x5D1) + b" " + enc(0x627) + enc(0x644) + b" 5" + enc(0xB2) + enc(0x2074) + b"\n",
    ]
    # every alignment: a two-byte and a General Punctuation character with its first byte at corpus positions 0..3 mod 4
    for k in range(4):
        docs.append(b"x" * k + E + b" then " + DASH + b"x" * k + QUOTE + b"s " + b"y" * k + E + E + DASH + DASH + E)
    have = sum(len(d) for d in docs)
    assert have < TILE - 40
    fill = (b"plain filler text up to the edge of the first tile, " * 20)[:TILE - 1 - have - 4]
    docs.append(fill + b" caf" + at_edge + b" and the second tile goes on with " + E + b"t" + E + b" " + DASH + b" more")
    tail = b"na" + enc(0xEF) + b"ve " + enc(0x201C) + b"r" + E + b"sum" + E + enc(0x201D) + b" " + DASH + b" S" + enc(0xE3) + b"o Paulo, Z" + enc(0xFC) + b"rich" + enc(0x2026) + b" "
    docs += [tail * 8, b"x" + tail * 8 + E, b"xy" + tail * 7 + DASH]          # (the corpus' last bytes: a character)
    blob = b"".join(docs)
    assert blob[TILE - 1:TILE - 1 + len(at_edge)] == at_edge and 2 * TILE < len(blob) <= 3000
    for ch in (E, DASH, QUOTE):                                                  # (self-check: every alignment is there)
        pos, i = set(), blob.find(ch)
        while i >= 0:
            pos.add(i % 4)
            i = blob.find(ch, i + 1)
        assert pos == {0, 1, 2, 3}, (ch, pos)
    return docs


@pytest.mark.parametrize("tables", ["pcre2", "regex"])
@pytest.mark.parametrize("name", ["cl100k_base", "o200k_base", "mistral_v3"])
def test_two_byte_text_cases(name, tables):
    from splintr_amd import Tokenizer
    t = Tokenizer.from_pretrained(name, unicode_tables=tables)
    orc = _oracle(name, tables)
    _profile(t, True)
    try:
        for what, at_edge in (("two-byte character on the tile boundary", E), ("General Punctuation on the tile boundary", DASH)):
            docs = _two_byte_docs(at_edge)
            b, want = _raw_batch(docs), _want(orc, docs)
            for fuse in (1, 0):
                _opt(t, "fuse", fuse)
                for p in range(2):                                               # (memo cold, then warm)
                    _same(_encode(t, b, "fused" if fuse else "two"), want, f"{name} {tables}: {what}, fuse {fuse}, pass {p}")
    finally:
        _profile(t, False)


# ------------------------------------------------------------------------------------------------
# the merge phase
# ------------------------------------------------------------------------------------------------
NAME = "cl100k_base"
WORDS = ("the of and to in is that for with as on by this from have not are but all would there their what about which when make like time "
         "just know take people into year your good some could them see other than then now look only come over think also back after use "
         "two how our work first well way even new want because any these give day most").split()
SHORT_MISS, MEDIUM_MISS = b" xqzvkwj", b" " + b"xqzvkwjhg" * 3          # 8 bytes, 28 bytes: letters only, one chunk each, no token


def _words(n_bytes, seed):
    """A document of exactly n_bytes of common words (every chunk a vocabulary token: checked in _misses)."""
    out, k = b"The", seed
    while True:
        w = b" " + WORDS[k % len(WORDS)].encode()
        if len(out) + len(w) > n_bytes:
            break
        out += w
        k = k * 7 + 3
    out += b" a" * ((n_bytes - len(out)) // 2)
    return out + b"." * (n_bytes - len(out))                                   # (at most one: a chunk of one byte is never a miss)


def _misses(docs):
    """Per tile: the lengths of the chunks of two bytes and more that START in it and are no single vocabulary token (the oracle's split)."""
    orc = _oracle(NAME)
    per_tile, base = {}, 0
    for d in docs:
        starts = list(orc.split_bytes(d)) + [len(d)]
        for a, z in zip(starts, starts[1:]):
            if z - a >= 2 and len(orc.encode_bytes(d[a:z])) != 1:
                per_tile.setdefault((base + a) // TILE, []).append(z - a)
        base += len(d)
    return per_tile


def _merge_batches():
    filler = [_words(200, s) for s in range(12)]                                 # 2 400 bytes: three tiles
    mid = lambda miss: filler[:5] + [_words(100, 40) + miss + b" " + _words(99 - len(miss), 41)] + filler[6:]   # (the miss at corpus byte 1 100)
    every = [_words(100, 50 + k) + MEDIUM_MISS + b" " + _words(200 - 101 - len(MEDIUM_MISS), 70 + k) for k in range(12)]
    return {
        "no tile has a miss": (filler, {}),
        "the middle tile has one short miss": (mid(SHORT_MISS), {1: [len(SHORT_MISS)]}),
        "the middle tile has one medium miss": (mid(MEDIUM_MISS), {1: [len(MEDIUM_MISS)]}),
        "every tile has medium misses only": (every, {0: [len(MEDIUM_MISS)] * 4, 1: [len(MEDIUM_MISS)] * 4, 2: [len(MEDIUM_MISS)] * 4}),
    }


def test_merge_batches_are_what_they_claim():
    """(no kernel runs here: the batches' misses, by the oracle's split and vocabulary)"""
    for what, (docs, misses) in _merge_batches().items():
        assert sum(len(d) for d in docs) == 3 * TILE, what
        assert _misses(docs) == misses, what
    assert 2 <= len(SHORT_MISS) <= 16 and 17 <= len(MEDIUM_MISS) <= 64


@pytest.mark.parametrize("fuse", [1, 0])
@pytest.mark.parametrize("memo", [1, 0])
def test_merge_skip(memo, fuse):
    from splintr_amd import Tokenizer
    t = Tokenizer.from_pretrained(NAME)
    orc = _oracle(NAME)
    _opt(t, "memo", memo)
    _opt(t, "fuse", fuse)
    _profile(t, True)
    try:
        for what, (docs, _) in _merge_batches().items():
            b, want = _raw_batch(docs), _want(orc, docs)
            _opt(t, "memo_clear", 1)
            for p in range(3 if memo else 1):                                    # memo on: cold, filling, warm
                _same(_encode(t, b, "fused" if fuse else "two"), want, f"{what}: memo {memo}, fuse {fuse}, pass {p}")
    finally:
        _profile(t, False)
