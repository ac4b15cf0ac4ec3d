"""The plain span reference (mode_spans_ref.py) off the GPU: its ids against wordpiece_ref / unigram_ref, its character spans against the
figures checked by hand and against Hugging Face's tokenizers where that module imports.  test_gpu_mode_spans.py takes the vocabularies
and the texts from here."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import mode_spans_ref as ref  # noqa: E402
import unigram_ref  # noqa: E402
import wordpiece_ref  # noqa: E402

# ---- WordPiece: test_gpu_wordpiece.py's vocabulary; a small one under which the checked cases split as they were checked
SINGLE = "abcdefghijklmnoprstuvwxyzABCXéèüeαβγσςбгджあア中文漢한글가각\u0301!#.,;-()$+§«»…0123456789"       # (no q)
WP_KEYS = list(dict.fromkeys(
    ["[PAD]", "[UNK]", "[CLS]", "[SEP]"] + list(SINGLE) + ["##" + c for c in dict.fromkeys(SINGLE) if c not in "!#.,;-()$+§«»…中文漢"]
    + ["ab", "abcd", "##cx", "xy", "##yq", "xq", "hello", "world", "##ld", "caf", "cafe", "##é", "한글", "##글한", "αβ", "##γ", "бг", "aaaa", "##aaa",
       "##", "#a", "the", "##ing", "token", "##izer", "##s"]))
WP_VOCAB = {k: i for i, k in enumerate(WP_KEYS)}
WP_SMALL = {k: i for i, k in enumerate(["[PAD]", "[UNK]", "hello", ",", "wor", "##ld", "cafe", "##s", "a", "##b", "e", "x", "i"])}
WP_CHECKED = [("Hello, world", [(0, 5), (5, 6), (7, 10), (10, 12)]), ("cafe\u0301s", [(0, 4), (5, 6)]), ("a\u200bb", [(0, 1), (2, 3)]),
              ("\u0301e", [(1, 2)]), ("  zzz  x", [(2, 5), (7, 8)]), ("İ", [(0, 1)])]
WP_LONG = ("hello world abcx xyq xqz cafe\u0301 Café naïve αβγ Σσς бгд ab中文cd tokenizers, the-tokening!! "
           "한글한글한 a\xadb x\u200by $5+3 «ab»… #a a# ## aaaaaaa あア qab abq " + "a" * 300 + " ") * 22       # ~10 KB: three normaliser tiles

# ---- Unigram: test_gpu_unigram.py's pieces; a small set under which the checked cases split as they were checked
UNI_PIECES = [("<unk>", 0.0), ("<s>", 0.0), ("</s>", 0.0), ("<pad>", 0.0), ("▁", -2.0), ("b", -3.5), ("ab", -6.5), ("c", -4.0), ("▁a", -4.5),
              ("▁ab", -8.0), ("é", -5.0), ("日", -5.5), ("本", -5.5), ("日本", -11.0), ("a\tb", -7.0), ("\t", -6.5), ("x", -6.0), ("xx", -12.0),
              ("z", -7.5), ("bc", -7.0), ("▁日", -8.0), ("cé", -8.5)] + [("a" * k, -3.0 * k) for k in range(1, 17)]
UNI_SMALL = [("<unk>", 0.0), ("▁", -2.0), ("▁hello", -5.0), ("▁wor", -4.0), ("ld", -3.0), ("▁a", -3.0), ("b", -2.0), ("a", -2.5)]
UNI_CHECKED = [("hello world", [(0, 5), (5, 9), (9, 11)]), (" hello", [(0, 6)]), ("é", [(0, 1), (0, 1)]), ("a  b", [(0, 1), (1, 2), (2, 3), (3, 4)]),
               ("aqqb", [(0, 1), (1, 3), (3, 4)]), ("hello ", [(0, 5), (5, 6)])]
UNI_LONG = ("ab c日本 zqz  ab▁日本céz é日 a\xadb 한글 qq▁q xxx " + "a" * 300 + " ") * 4                    # ~1.6 KB: three tiles of 512


def wp_hf(vocab, lowercase=True, strip_accents=None):
    tk = pytest.importorskip("tokenizers")
    hf = tk.Tokenizer(tk.models.WordPiece(vocab, unk_token="[UNK]", max_input_chars_per_word=100))
    hf.normalizer = tk.normalizers.BertNormalizer(clean_text=True, handle_chinese_chars=True, strip_accents=strip_accents, lowercase=lowercase)
    hf.pre_tokenizer = tk.pre_tokenizers.BertPreTokenizer()
    return hf


def uni_hf(pieces, prepend):
    tk = pytest.importorskip("tokenizers")
    hf = tk.Tokenizer(tk.models.Unigram([(p, s) for p, s in pieces], unk_id=0, byte_fallback=False))
    hf.pre_tokenizer = tk.pre_tokenizers.Metaspace(replacement="▁", prepend_scheme=prepend)
    return hf


@pytest.mark.parametrize("text,chars", WP_CHECKED, ids=[repr(t) for t, _ in WP_CHECKED])
def test_wordpiece_checked(text, chars):
    ids, spans = ref.wordpiece_spans(text.encode(), WP_SMALL, 1)
    assert ids == wordpiece_ref.encode(text, WP_SMALL, 1) and ref.to_chars(text.encode(), spans) == chars
    enc = wp_hf(WP_SMALL).encode(text, add_special_tokens=False)
    assert (enc.ids, enc.offsets) == (ids, chars)


@pytest.mark.parametrize("text,chars", UNI_CHECKED, ids=[repr(t) for t, _ in UNI_CHECKED])
def test_unigram_checked(text, chars):
    ids, spans = ref.unigram_spans(text.encode(), UNI_SMALL, 0, "always")
    assert ids == unigram_ref.encode(text, UNI_SMALL, 0, "always") and ref.to_chars(text.encode(), spans) == chars
    enc = uni_hf(UNI_SMALL, "always").encode(text, add_special_tokens=False)
    assert (enc.ids, enc.offsets) == (ids, chars)


@pytest.mark.parametrize("lowercase,strip_accents", [(True, None), (False, False)])
def test_wordpiece_long_text(lowercase, strip_accents):
    """The GPU test's vocabulary and text: every script, dropped code points, a word over the limit."""
    doc = WP_LONG[:1200].encode()
    ids, spans = ref.wordpiece_spans(doc, WP_VOCAB, 1, lowercase=lowercase, strip_accents=strip_accents)
    assert ids == wordpiece_ref.encode(doc, WP_VOCAB, 1, lowercase=lowercase, strip_accents=strip_accents)
    enc = wp_hf(WP_VOCAB, lowercase, strip_accents).encode(doc.decode(), add_special_tokens=False)
    assert (enc.ids, enc.offsets) == (ids, ref.to_chars(doc, spans))


@pytest.mark.parametrize("prepend", ["always", "never"])
def test_unigram_long_text(prepend):
    doc = UNI_LONG[:500].encode()
    ids, spans = ref.unigram_spans(doc, UNI_PIECES, 0, prepend)
    assert ids == unigram_ref.encode(doc, UNI_PIECES, 0, prepend)
    enc = uni_hf(UNI_PIECES, prepend).encode(doc.decode(), add_special_tokens=False)
    assert (enc.ids, enc.offsets) == (ids, ref.to_chars(doc, spans))


def test_ill_formed_bytes_are_no_source():
    doc = b"ab\xffcd \xe2\x82 x"
    assert ref.wordpiece_spans(doc, WP_VOCAB, 1) == (wordpiece_ref.encode(doc, WP_VOCAB, 1), [(0, 5), (9, 10)])       # abcd, around the byte
    ids, spans = ref.unigram_spans(doc, UNI_PIECES, 0, "never")
    assert ids == unigram_ref.encode(doc, UNI_PIECES, 0, "never") and spans[:3] == [(0, 2), (2, 3), (3, 4)]
