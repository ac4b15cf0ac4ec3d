"""spl_encode_batch_spans_device on the GPU (k_wp_norm<write, map>, k_wp_match<write, span>, k_uni_match / k_uni_long<write, span>,
k_text_cstarts): ids and spans, exact, against the plain reference (mode_spans_ref.py), per mode and per unit.  Tiles: the normaliser's
4 096 bytes, the matcher's 2 048, Unigram's 512 with a halo of 128, the character count's 64."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import mode_spans_ref as ref  # noqa: E402
from test_mode_spans_cpu import UNI_CHECKED, UNI_LONG, UNI_PIECES, WP_CHECKED, WP_KEYS, WP_LONG, WP_VOCAB  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# WordPiece (lowercase, strip_accents, max_input_chars_per_word): the default, nothing folded, a cheap word limit; Unigram: prepend_scheme
MODES = [("wp", (True, None, 100)), ("wp", (False, False, 100)), ("wp", (True, None, 4)), ("uni", "always"), ("uni", "never")]


class Mode:
    def __init__(self, kind, opt):
        from splintr_amd import Tokenizer
        self.kind, self.opt = kind, opt
        if kind == "wp":
            self.tok = Tokenizer.from_bytes_wordpiece("\n".join(WP_KEYS).encode() + b"\n", lowercase=opt[0], strip_accents=opt[1],
                                                      max_input_chars_per_word=opt[2])
        else:
            self.tok = Tokenizer.from_bytes_unigram(UNI_PIECES, 0, prepend_scheme=opt)
        self.want = functools.lru_cache(maxsize=None)(self._want)

    def _want(self, doc):
        if self.kind == "wp":
            return ref.wordpiece_spans(doc, WP_VOCAB, 1, self.opt[2], lowercase=self.opt[0], strip_accents=self.opt[1])
        return ref.unigram_spans(doc, UNI_PIECES, 0, self.opt)

    def wants(self, docs, unit):
        """[(ids, spans)] per document in the unit asked for."""
        return [(i, ref.to_chars(d, s) if unit == "char" else s) for d in docs for i, s in [self.want(d)]]


@pytest.fixture(scope="module", params=MODES, ids=lambda m: f"{m[0]}-{m[1]}")
def mode(request):
    return Mode(*request.param)


def as_bytes(docs):
    return [d.encode() if isinstance(d, str) else d for d in docs]


def spans_call(mode, docs, unit, short=0):
    """One device call with the span buffer of `unit` alone: ([(ids, spans)] per document, cut at the capacity; the need).  The rows at and
    beyond the capacity must keep their sentinel."""
    from splintr_amd import _ffi
    buf = b"".join(docs)
    off = np.cumsum([0] + [len(d) for d in docs]).astype(np.int64)
    text = torch.from_numpy(np.frombuffer(buf + b"\xe2" * ((-len(buf)) % 16 + 16), dtype=np.uint8).copy()).cuda()
    d_off, out_off = torch.from_numpy(off).cuda(), torch.full((len(docs) + 1,), -1, dtype=torch.int64, device="cuda")
    cap = max(sum(len(mode.want(d)[0]) for d in docs) - short, 0)
    ids = torch.full((cap + 8,), -7, dtype=torch.int32, device="cuda")
    span = torch.full((cap + 8, 2), -7, dtype=torch.int32, device="cuda")
    rc = _ffi.lib().spl_encode_batch_spans_device(mode.tok.handle, text.data_ptr(), len(buf), d_off.data_ptr(), len(docs), 0, ids.data_ptr(), cap,
                                                  out_off.data_ptr(), span.data_ptr() if unit == "byte" else None,
                                                  span.data_ptr() if unit == "char" else None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _ffi.last_error()
    oo, flat, sp = out_off.cpu().tolist(), ids.cpu().tolist(), [tuple(r) for r in span.cpu().tolist()]
    assert flat[cap:] == [-7] * 8 and sp[cap:] == [(-7, -7)] * 8, "stored at or beyond ids_capacity"
    return [(flat[oo[i]:min(oo[i + 1], cap)], sp[oo[i]:min(oo[i + 1], cap)]) for i in range(len(docs))], oo[-1]


CASES = {
    "checked": [t for t, _ in WP_CHECKED + UNI_CHECKED],
    "empty_between_full": ["", "hello world", "", "", "a  b", "", "café ab", ""],
    "only_dropped": ["\x00\u200b\ufeff", "ab", "\u200b", "\xad\xad", "cd"],
    "ill_formed": [b"ab\xffcd \xe2\x82 x", b"a\xe2\x82", b"\xacb", b"\x80\x80ab\xe2", b"\xe6\x97\xa5\xe6\x97 ab\xc3"],
    # Unigram: words longer than the halo, one with the prepended marker, one that starts just in front of a tile edge and ends in unk;
    # WordPiece: an unk word that ends beyond the matcher's halo
    "long_words": ["a" * 700 + " b", ("ab c " * 102)[:508] + " " + "ab" * 100 + "qqq日本" * 30 + "q c", "xq" * 1200 + "é ab", "ab " + "é" * 600],
    "thousand_docs": [("ab cé q日本 xyq ".encode() * (i % 5))[: i % 23] for i in range(1000)],       # (some end inside a character)
}


@pytest.mark.parametrize("unit", ["byte", "char"])
@pytest.mark.parametrize("case", list(CASES))
def test_device_call(mode, case, unit):
    docs = as_bytes(CASES[case])
    got, need = spans_call(mode, docs, unit)
    assert got == mode.wants(docs, unit)
    assert need == sum(len(i) for i, _ in got)


@pytest.mark.parametrize("unit", ["byte", "char"])
@pytest.mark.parametrize("shift", range(17))
def test_tile_edges(mode, shift, unit):
    """Every word and every multi-byte source of a text of three tiles meets each tile's edge and a 64-byte block's at some shift."""
    docs = as_bytes(["z" * shift + (WP_LONG if mode.kind == "wp" else UNI_LONG)])
    got, _ = spans_call(mode, docs, unit)
    assert got == mode.wants(docs, unit)


@pytest.mark.parametrize("unit", ["byte", "char"])
def test_capacity_one_short(mode, unit):
    docs = as_bytes(["hello world", WP_LONG[:300], "ab cé"])
    full = mode.wants(docs, unit)
    got, need = spans_call(mode, docs, unit, short=1)
    assert need == sum(len(i) for i, _ in full)
    assert got == full[:2] + [(full[2][0][:-1], full[2][1][:-1])]


def test_refusals(mode):
    from splintr_amd import Tokenizer, _ffi
    z = torch.zeros(64, dtype=torch.int64, device="cuda")
    call = lambda h, b, c: _ffi.lib().spl_encode_batch_spans_device(h, z.data_ptr(), 0, z.data_ptr(), 1, 0, z.data_ptr(), 8, z.data_ptr(), b, c, None)  # noqa: E731
    assert call(mode.tok.handle, None, None) == -1 and "both null" in _ffi.last_error()
    assert call(mode.tok.handle, z.data_ptr() + 4, None) == -1 and "8-byte aligned" in _ffi.last_error()
    assert call(Tokenizer.from_pretrained("cl100k_base").handle, z.data_ptr(), None) == -1 and "spl_token_spans_device" in _ffi.last_error()


@pytest.mark.parametrize("unit", ["byte", "char"])
def test_encode_batch_with_offsets(mode, unit):
    """The Python surface: ValueError (ids that do not decode to the text) or NotImplementedError without the span kernels."""
    texts = ["Hello, world", "", "cafe\u0301s a\u200bb", "b", "hello ", (WP_LONG if mode.kind == "wp" else UNI_LONG)[:700]]
    ids, spans = mode.tok.encode_batch_with_offsets(texts, unit=unit)
    want = mode.wants(as_bytes(texts), unit)
    assert ids == [i for i, _ in want] and spans == [s for _, s in want]
