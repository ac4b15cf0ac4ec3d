"""GPU tests (-m gpu) of the form for the two words that one two-byte character straddles (word_straddle / classify_word_straddle,
csrc/spl_scan_words.h) inside k_pretok -- the lead 110xxxxx in byte 3 of a four-byte word, the continuation in byte 0 of the next --
and of the words next to them that keep the older paths: every result bit-exact on ids and offsets against oracle.coracle.COracle.
Small shapes, each where the form or its gate can go wrong:

  sentences    documents of about 40 bytes, a few hundred a batch: an ASCII sentence with e-acute (a letter) or the multiplication sign
               (class "other") whose lead byte falls on byte 3 of a word -- as the document's first and last character, at distances
               1..7 from its start and from its end, with a space, an apostrophe, a digit and a newline directly before and behind
               it, two such characters in consecutive words (a word with the continuation in byte 0 AND a lead in byte 3), and one
               beside an "inside" character in the same 256-byte stretch
  tiles        two documents of 1000 bytes, the lead at corpus bytes 799 and 1599 (the continuation is the first byte of the next
               tile's own range) and at 767 and 1567 (the continuation is window index 0 of the next tile: no word in front); the lead
               on the last byte of the corpus' last full word with the corpus ending right behind the continuation, and ending ON the
               lead (a truncated character)
  documents    a document boundary between the lead and the continuation, directly before the lead, and directly behind the
               continuation, the neighbouring documents one and two bytes long
  special      a special-token literal ending directly before the lead and starting directly behind the continuation, through the
               special-token encode

Three vocabularies; one launch and two; memo cold, then warm."""
import json
import os

import numpy as np
import pytest

from test_gpu_fused import _opt, _poison, _same
from test_gpu_warm_tile_path import _oracle, _raw_batch, enc

pytestmark = pytest.mark.gpu

NAMES = ["cl100k_base", "o200k_base", "mistral_v3"]
CHARS = {"e-acute": enc(0xE9), "multiplication sign": enc(0xD7)}
S1 = b"The quick brown fox jumps over the lazy dog again"
S2 = b"it's 12 o'clock, isn't it? 3 times 4 makes 12 now"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_toks = {}


def _tok(name):
    from splintr_amd import Tokenizer
    if name not in _toks:
        _toks[name] = Tokenizer.from_pretrained(name)
    return _toks[name]


def _want(orc, docs, special=False):
    off = np.zeros(len(docs) + 1, dtype=np.uint64)
    np.cumsum([len(d) for d in docs], out=off[1:])
    return orc.encode_packed(np.frombuffer(b"".join(docs), dtype=np.uint8), off, special, threads=8)


def _check(name, docs, what, special=False):
    """The batch as one launch and as two, memo cold then warm, against the oracle."""
    import torch
    from splintr_amd.device import encode_device, result_csr
    t, want = _tok(name), _want(_oracle(name), docs, special)
    b = _raw_batch(docs)
    try:
        for fuse in (1, 0):
            _opt(t, "fuse", fuse)
            _opt(t, "memo_clear", 1)
            for p in range(2):
                _poison(b)
                encode_device(t, b, special)
                torch.cuda.synchronize()
                _same(result_csr(b), want, f"{name}: {what}, fuse {fuse}, pass {p}")
    finally:
        _opt(t, "fuse", 1)


class _Batch:
    """Documents in a row; a case is put so that the byte behind `before` falls on byte k of a four-byte word (the corpus begins a word,
    and so does every window: tile starts and the halo are multiples of four), by a short document of padding in front."""

    def __init__(self):
        self.docs, self.n, self.seen = [], 0, set()

    def add(self, tag, before, ch, behind, k=3):
        pad = (k - self.n - len(before)) % 4
        if pad:
            self._put(b"pad."[:pad])
        assert (self.n + len(before)) % 4 == k
        self.seen.add(tag)
        self._put(before + ch + behind)

    def _put(self, d):
        self.docs.append(d)
        self.n += len(d)


TAGS = (["first", "last"] + [f"start+{d}" for d in range(1, 8)] + [f"end-{d}" for d in range(1, 8)] +
        [f"around {nb!r}" for nb in (b" ", b"'", b"7", b"\n")] + ["consecutive 2", "consecutive 3", "beside inside"])


def _sentence_docs(ch):
    b = _Batch()
    for s in (S1, S2):
        b.add("first", b"", ch, s[:38])
        b.add("last", s[:38], ch, b"")
        for d in range(1, 8):
            b.add(f"start+{d}", s[:d], ch, s[d:36])
            b.add(f"end-{d}", s[:36 - d], ch, s[36 - d:36])
        for nb in (b" ", b"'", b"7", b"\n"):
            b.add(f"around {nb!r}", s[:17] + nb, ch, nb + s[17:34])
        # leads on byte 3 of consecutive words: the word between them has the continuation in byte 0 AND a lead in byte 3
        b.add("consecutive 2", s[:9], ch + b"aa" + ch + s[9:30], b"")
        b.add("consecutive 3", s[:9], ch + b"aa" + ch + b"ab" + ch + s[9:26], b"")
        # an "inside" character (lead on byte 1) in the word behind the continuation's, same document
        b.add("beside inside", s[:9], ch + s[9:13] + ch + s[13:32], b"")
    return b


@pytest.mark.parametrize("ch", list(CHARS))
def test_sentence_batches_are_what_they_claim(ch):
    """(no kernel runs here)"""
    c = CHARS[ch]
    b = _sentence_docs(c)
    assert b.seen == set(TAGS)
    assert 40 <= len(b.docs) <= 120 and max(len(d) for d in b.docs) <= 44 and b.docs[:2] == [b"pad", c + S1[:38]] and c + b"aa" + c + b"ab" + c in b"".join(b.docs)
    blob = b"".join(b.docs)
    at = [i % 4 for i in range(len(blob)) if blob.startswith(c, i)]
    assert at.count(3) >= 2 * (len(TAGS) + 3) and 1 in at                  # every case a lead on byte 3; the "inside" one beside it
    w = [blob[i:i + 4] for i in range(0, len(blob) - 3, 4)]
    assert sum(1 for x in w if x[0] == c[1] and x[3] == c[0]) >= 6         # both alignments in one word


@pytest.mark.parametrize("ch", list(CHARS))
@pytest.mark.parametrize("name", NAMES)
def test_sentences(name, ch):
    _check(name, _sentence_docs(CHARS[ch]).docs, f"sentences with {ch}")


def _tile_docs(leads, n=2000):
    """Documents of 1000 bytes (the last one shorter: n bytes in all); leads at the given corpus bytes."""
    src = (S1 + b" " + S2 + b"\n") * 21
    chs = [CHARS["e-acute"], CHARS["multiplication sign"]] * 3
    blob = b""
    for a, c in zip(leads, chs):
        blob += src[len(blob):a] + c
    blob = (blob + src[len(blob):n])[:n]
    assert len(blob) == n and all(blob[a:a + 2] == c[:n - a] for a, c in zip(leads, chs))
    return [blob[:1000], blob[1000:]]


def test_tile_batches_are_what_they_claim():
    """(no kernel runs here)"""
    d = _tile_docs([767, 799, 1567, 1599])
    blob = b"".join(d)
    assert [len(x) for x in d] == [1000, 1000] and all(blob[a] in (0xC3,) and blob[a + 1] in (0xA9, 0x97) for a in (767, 799, 1567, 1599))
    d = _tile_docs([767, 799, 1567, 1599, 1799], 1801)
    assert sum(map(len, d)) == 1801 and b"".join(d)[-2:] == CHARS["e-acute"]
    d = _tile_docs([767, 799, 1567, 1599, 1799], 1800)
    assert sum(map(len, d)) == 1800 and b"".join(d)[-1] == 0xC3 and 1799 % 4 == 3


@pytest.mark.parametrize("name", NAMES)
def test_tile_boundaries_and_the_halo_edge(name):
    _check(name, _tile_docs([767, 799, 1567, 1599]), "leads at 767, 799, 1567, 1599")
    _check(name, _tile_docs([767, 799, 1567, 1599, 1799], 1801), "the corpus ends right behind the continuation")
    _check(name, _tile_docs([767, 799, 1567, 1599, 1799], 1800), "the corpus ends ON the lead")


def _boundary_docs():
    b = _Batch()
    for ch in CHARS.values():
        for n in (1, 2):                                          # the neighbouring document: one byte, two bytes
            nb = b"ab"[:n]
            b.add(f"before {n}", b"", ch, b" follows")               # a boundary directly before the lead ...
            b._put(nb)
            b.add(f"before' {n}", b"", ch, b"")                      # ... behind a short document; the character a document
            b._put(nb)
            b.add(f"behind {n}", b"caf", ch, b"")                    # a boundary directly behind the continuation, a short document next
            b._put(nb)
            b.add(f"between {n}", b"caf", ch[:1], b"")               # a boundary between the lead and its continuation
            b._put(ch[1:] + b" au lait")
            b.add(f"between' {n}", nb[:n - 1], ch[:1], b"")          # ... the lead (with one byte in front) a document ...
            b._put(ch[1:] + nb[:n - 1])                              # ... and the continuation one
            b._put(b" and on")
    return b


def test_boundary_batch_is_what_it_claims():
    """(no kernel runs here)"""
    b = _boundary_docs()
    assert b.seen == {f"{t} {n}" for t in ("before", "before'", "behind", "between", "between'") for n in (1, 2)}
    assert b"\xC3" in b.docs and b"\xA9" in b.docs and b"a\xC3" in b.docs and b"\x97a" in b.docs
    blob = b"".join(b.docs)
    assert all(i % 4 == 3 for i in range(len(blob)) if blob[i] == 0xC3)


@pytest.mark.parametrize("name", NAMES)
def test_document_boundaries(name):
    _check(name, _boundary_docs().docs, "document boundaries at the straddling character")


@pytest.mark.parametrize("name", NAMES)
def test_special_literals_around_the_letter(name):
    with open(os.path.join(ROOT, "splintr_amd", "data", "special_tokens.json"), encoding="utf-8") as f:
        lits = [x.encode() for x in json.load(f)[name]]
    lit = max(lits[:4], key=len)
    b = _Batch()
    for ch in CHARS.values():
        b.add("both", b"caf" + lit, ch, lit + b" x")
        b.add("before", lit, ch, b"t" + ch)
        b.add("behind", b"a", ch, lit)
        b.add("between", b"a", ch[:1], lit + ch[1:] + b"z")           # (a literal between the lead and its continuation)
    assert b.seen == {"both", "before", "behind", "between"}
    _check(name, b.docs, "special literals at the straddling letter", special=True)
    _check(name, b.docs, "the same text without the special-token scan")
