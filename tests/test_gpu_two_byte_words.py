"""GPU tests (-m gpu) of the two-byte form of the word classifier (classify_word_two, csrc/spl_scan_words.h) inside k_pretok<800,192>,
every result compared with the oracle.  What tests/test_gpu_warm_tile_path.py::test_two_byte_text_cases does not have:

  runs        40 and more Cyrillic and Greek letters in a row -- every word [L C L C] or [C L C L] -- starting at corpus bytes 0..3 mod 4
  straddle    a two-byte letter whose lead byte is the last byte of a wavefront's quarter of the window and whose continuation byte is the
              first of the next one: window indices 255 | 256, 511 | 512, 767 | 768 of every tile (window index = corpus byte - 800 * tile + 32)
  edges       a document that is one two-byte character; documents of 1..3 ASCII bytes between two such documents (a text start within
              three bytes: the guard declines); a two-byte character directly behind and in front of a three-byte and a four-byte one;
              lead behind lead; the corpus ending on a lead byte

Every batch is three tiles of 800 bytes; three vocabularies, both Unicode tables, as one launch and as two, memo cold then warm."""
import pytest

from test_gpu_fused import _encode, _opt, _profile, _same
from test_gpu_warm_tile_path import TILE, _oracle, _raw_batch, _want, enc

pytestmark = pytest.mark.gpu

LH = 32                                                    # the window's left halo: window index 0 is corpus byte 800 * tile - 32
E, DASH, EMOJI = enc(0xE9), enc(0x2014), b"\xF0\x9F\x98\x80"
CYRILLIC = b"".join(enc(0x430 + k % 32) for k in range(44))          # 44 lower-case letters, 88 bytes
GREEK = b"".join(enc(0x3B1 + k % 24) for k in range(41))             # 41 letters, 82 bytes (final sigma among them)
FILL = b"plain filler text between the cases, with a number 12345 and it's punctuation; "


def _pad_to(blob, k):
    """ASCII behind `blob` until its length is k mod 4 (a space first, so that what follows starts a word)."""
    out = b" "
    while (len(blob) + len(out)) % 4 != k:
        out += b"x"
    return out


def _fill(docs, lo=2 * TILE + 1, hi=3 * TILE):
    """A last document of filler (with accented letters in it) so that the batch is three tiles."""
    have = sum(len(d) for d in docs)
    assert have < hi - 8, have
    tail = (FILL + b"na" + enc(0xEF) + b"ve caf" + E + b" ") * 40
    docs.append(tail[:max(lo + 40 - have, 8)])
    if docs[-1][-1] >= 0xC0:                                # (not ending on a lead byte by accident: that is a case of its own)
        docs[-1] = docs[-1][:-1]
    n = sum(len(d) for d in docs)
    assert lo <= n <= hi, n
    return docs


def _runs_batch():
    docs, blob = [], b""
    for k in range(4):
        for run in (CYRILLIC, GREEK):
            d = b"go" + _pad_to(blob + b"go", k)
            assert (len(blob) + len(d)) % 4 == k
            d += run + b" and " + run[:6] + b"."
            docs.append(d)
            blob += d
    starts = {(s, blob.find(run, at) % 4) for s, run in (("cyrillic", CYRILLIC), ("greek", GREEK)) for at in range(len(blob)) if blob.startswith(run, at)}
    assert starts == {(s, k) for s in ("cyrillic", "greek") for k in range(4)}, starts
    return _fill(docs)


def _straddle_batch():
    """One blob of three tiles with a two-byte letter on every wavefront boundary of every tile's window, cut into documents away from them."""
    want_at = sorted(TILE * t - LH + q for t in range(3) for q in (255, 511, 767))      # corpus byte of the lead
    letters = [E, enc(0x436), enc(0x3B1), enc(0xF1), enc(0xC5), enc(0x5D0), enc(0xFC), enc(0x44F), enc(0xE7)]
    blob, src = b"", FILL * 40
    for at, ch in zip(want_at, letters):
        blob += src[len(blob):at] + ch
    blob += src[len(blob):3 * TILE - 7]
    for at, ch in zip(want_at, letters):
        assert blob[at:at + 2] == ch and (at - TILE * (at // TILE) + LH) % 256 == 255
    assert 2 * TILE < len(blob) <= 3 * TILE
    cuts = [0, 100, 101, 700, 1300, 1301, 1302, 2000, len(blob)]                       # (none within eight bytes of a boundary letter)
    assert all(abs(c - at) > 8 for c in cuts for at in want_at)
    return [blob[a:z] for a, z in zip(cuts, cuts[1:])]


def _edges_batch():
    docs = []
    for k in range(4):
        docs += [b"pad" + b"x" * k + b" ", E, b"a", E, b"ab", enc(0x436), b"abc", E, E, E + b"a" + E, b"a" + E, E + b"ab"]
        docs += [b"x" * k + DASH + E + DASH + b" " + EMOJI + E + EMOJI + b" " + E + DASH + E + b" " + E + EMOJI + E + b" "]
        docs += [b"y" * k + b"\xC3\xC3\xA9 a\xD0\xC3\xA9b \xC3" + E + E + b" \xD0\xD0\xD0\xB6"]                 # lead behind lead
    docs = _fill(docs, hi=3 * TILE - 8)
    docs.append(b" the corpus ends on a lead caf\xC3")
    assert 2 * TILE < sum(len(d) for d in docs) <= 3 * TILE and docs[-1][-1] == 0xC3
    return docs


BATCHES = {"runs": _runs_batch, "straddle": _straddle_batch, "edges": _edges_batch}


def test_batches_are_what_they_claim():
    """(no kernel runs here)"""
    for what, make in BATCHES.items():
        docs = make()
        assert 2 * TILE < sum(len(d) for d in docs) <= 3 * TILE, what
    edges = _edges_batch()
    assert E in edges and edges.count(b"a") == 4 and edges.count(b"ab") == 4 and edges.count(b"abc") == 4


@pytest.mark.parametrize("tables", ["pcre2", "regex"])
@pytest.mark.parametrize("name", ["cl100k_base", "o200k_base", "mistral_v3"])
def test_two_byte_words(name, tables):
    from splintr_amd import Tokenizer
    t = Tokenizer.from_pretrained(name, unicode_tables=tables)
    orc = _oracle(name, tables)
    _profile(t, True)
    try:
        for what, make in BATCHES.items():
            docs = make()
            b, want = _raw_batch(docs), _want(orc, docs)
            for fuse in (1, 0):
                _opt(t, "fuse", fuse)
                _opt(t, "memo_clear", 1)
                for p in range(2):                                               # (memo cold, then warm)
                    _same(_encode(t, b, "fused" if fuse else "two"), want, f"{name} {tables}: {what}, fuse {fuse}, pass {p}")
    finally:
        _profile(t, False)
