"""GPU tests (-m gpu) of the form for the word that holds one whole two-byte character (word_inside / classify_word_inside,
csrc/spl_scan_words.h) inside k_pretok, and of the words next to it that keep the older paths: every result bit-exact on ids and
offsets against oracle.coracle.COracle.  Small shapes, each where the form or its gate can go wrong:

  sentences    documents of about 40 bytes, a few hundred a batch: an ASCII sentence with e-acute (a letter) or the multiplication sign
               (class "other") whose lead byte falls on byte 0, 1, 2 and 3 of a four-byte word -- as the document's first character, at
               distances 1..7 from its start and from its end, and with a space, an apostrophe, a digit and a newline directly before
               and behind it
  tiles        two documents of 1000 bytes, the character's lead at corpus bytes 797..803 and 1597..1603 (the 800-byte tile boundaries)
               and at 765..771 and 1565..1571 (window index 0 of the next tile: the edge of its left halo)
  documents    a document boundary directly before, inside and directly behind the character's two bytes, the neighbouring documents
               one and two bytes long
  special      a special-token literal directly before and behind the letter, through the special-token encode

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
    """Documents in a row; a case is put so that its character's lead byte falls on byte k of a four-byte word (the corpus begins a
    word, and so does every window: tile starts and the halo are multiples of four), by a short document of padding in front."""

    def __init__(self):
        self.docs, self.n, self.seen = [], 0, set()

    def add(self, tag, before, ch, behind, k):
        pad = (k - self.n - len(before)) % 4
        if pad:
            self._put(b"pad."[:pad])
        assert (self.n + len(before)) % 4 == k
        self.seen.add((tag, k))
        self._put(before + ch + behind)

    def _put(self, d):
        self.docs.append(d)
        self.n += len(d)


def _sentence_docs(ch):
    b = _Batch()
    for s in (S1, S2):
        for k in (0, 1, 2, 3):                                    # (the first case: the first character of the corpus, k = 0)
            b.add("first", b"", ch, s[:38], k)
            for d in range(1, 8):
                b.add(f"start+{d}", s[:d], ch, s[d:36], k)
                b.add(f"end-{d}", s[:36 - d], ch, s[36 - d:36], k)
            for nb in (b" ", b"'", b"7", b"\n"):
                b.add(f"around {nb!r}", s[:17] + nb, ch, nb + s[17:34], k)
    return b


@pytest.mark.parametrize("ch", list(CHARS))
def test_sentence_batches_are_what_they_claim(ch):
    """(no kernel runs here)"""
    b = _sentence_docs(CHARS[ch])
    tags = ["first"] + [f"start+{d}" for d in range(1, 8)] + [f"end-{d}" for d in range(1, 8)] + [f"around {nb!r}" for nb in (b" ", b"'", b"7", b"\n")]
    assert b.seen == {(t, k) for t in tags for k in range(4)}
    assert 200 <= len(b.docs) <= 400 and max(len(d) for d in b.docs) <= 44 and b.docs[0].startswith(CHARS[ch])
    blob = b"".join(b.docs)
    assert {i % 4 for i in range(len(blob)) if blob.startswith(CHARS[ch], i)} == {0, 1, 2, 3}


@pytest.mark.parametrize("ch", list(CHARS))
@pytest.mark.parametrize("name", NAMES)
def test_sentences(name, ch):
    _check(name, _sentence_docs(CHARS[ch]).docs, f"sentences with {ch}")


def _tile_docs(j):
    """Two documents of 1000 bytes; leads at 768 + j, 800 + j, 1568 + j, 1600 + j."""
    src = (S1 + b" " + S2 + b"\n") * 21
    at = [768 + j, 800 + j, 1568 + j, 1600 + j]
    chs = [CHARS["e-acute"], CHARS["multiplication sign"], CHARS["multiplication sign"], CHARS["e-acute"]]
    blob = b""
    for a, c in zip(at, chs):
        blob += src[len(blob):a] + c
    blob += src[len(blob):2000]
    assert len(blob) == 2000 and all(blob[a:a + 2] == c for a, c in zip(at, chs)) and blob.count(b"\xC3") == 4
    return [blob[:1000], blob[1000:]]


@pytest.mark.parametrize("name", NAMES)
def test_tile_boundaries_and_the_halo_edge(name):
    for j in range(-3, 4):
        _check(name, _tile_docs(j), f"lead at 800 {j:+d}")


def _boundary_docs():
    b = _Batch()
    for ch in CHARS.values():
        for k in (0, 1, 2, 3):
            for n in (1, 2):                                      # the neighbouring document: one byte, two bytes
                nb = b"ab"[:n]
                b.add(f"before {n}", b"", ch, b" follows", k)            # a boundary directly before the character ...
                b._put(nb)
                b.add(f"before' {n}", b"", ch, b"", k)                   # ... behind a short document; the character a document
                b._put(nb)
                b.add(f"behind {n}", b"caf", ch, b"", k)                 # a boundary directly behind it, a short document next
                b._put(nb)
                b.add(f"inside {n}", b"caf", ch[:1], b"", k)             # a boundary between the lead and its continuation
                b._put(ch[1:] + b" au lait")
                b.add(f"inside' {n}", nb[:n - 1], ch[:1], b"", k)        # ... the lead (with one byte in front) a document ...
                b._put(ch[1:] + nb[:n - 1])                              # ... and the continuation one
                b._put(b" and on")
    return b


def test_boundary_batch_is_what_it_claims():
    """(no kernel runs here)"""
    b = _boundary_docs()
    assert b.seen == {(f"{t} {n}", k) for t in ("before", "before'", "behind", "inside", "inside'") for n in (1, 2) for k in range(4)}
    assert b"\xC3" in b.docs and b"\xA9" in b.docs and b"a\xC3" in b.docs and b"\x97a" in b.docs


@pytest.mark.parametrize("name", NAMES)
def test_document_boundaries(name):
    _check(name, _boundary_docs().docs, "document boundaries at the character")


@pytest.mark.parametrize("name", NAMES)
def test_special_literals_around_the_letter(name):
    with open(os.path.join(ROOT, "splintr_amd", "data", "special_tokens.json"), encoding="utf-8") as f:
        lits = [x.encode() for x in json.load(f)[name]]
    lit = max(lits[:4], key=len)
    b = _Batch()
    for ch in CHARS.values():
        for k in (0, 1, 2, 3):
            b.add("both", b"caf" + lit, ch, lit + b" x", k)
            b.add("before", lit, ch, b"t" + ch, k)
            b.add("behind", b"a", ch, lit, k)
            b.add("inside", b"a", ch[:1], lit + ch[1:] + b"z", k)        # (a literal between the lead and its continuation)
    assert b.seen == {(t, k) for t in ("both", "before", "behind", "inside") for k in range(4)}
    _check(name, b.docs, "special literals at the letter", special=True)
    _check(name, b.docs, "the same text without the special-token scan")
