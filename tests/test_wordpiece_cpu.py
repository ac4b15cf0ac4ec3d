"""WordPiece mode off the GPU: the product's table (splintr_amd/wordpiece.py) against the plain reference (wordpiece_ref.py), both
against Hugging Face's tokenizers where that module imports, the table builder's assertions, and the vocab.txt refusals."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import wordpiece_ref as ref  # noqa: E402
from splintr_amd import wordpiece as wp  # noqa: E402

# Latin with accents, Greek, Cyrillic, kana, Han, Hangul, punctuation and symbols, every whitespace kind, controls, U+0000, U+FFFD,
# soft hyphen, ZWSP, BOM, combining marks, U+1D160, emoji
POOL = ("abcxyzABCXYZ019" "àéîõüÅÇÑİſ" "αβγΣςΩΆ" "бгджЖЙЁ" "あいアイ" "中文漢字" "한글가힣" "!#.,;-_()[]{}'\"«»¿¡…—†$+<=>^`|~§©" "\u037e"
        " \t\n\r\x0b\x0c\x85\xa0\u1680 \u200a\u2028\u2029\u202f\u205f\u3000" "\x00\x01\x1f\x7f\ufffd\xad\u200b\ufeff"
        "\u0301\u0308\u0327\u0345\U0001d160😀🌍")
FIXED = ["", " ", "Hello, World!", "naïve café", "e\u0301lève", "ΑΘΗΝΑ Σοφός", "中文abc漢字", "a\xadb", "x\u200by", "\x00\ufffd",
         "한국어 텍스트", "a\u037eb", "\U0001d160x", "İstanbul ǅ ß ſ", "a" * 99, "b" * 100, "c" * 101, "d" * 150]
OPTS = [(lc, sa) for lc in (True, False) for sa in (True, False)]


def draw(seed, n):
    rng = random.Random(seed)
    return ["".join(rng.choice(POOL) for _ in range(rng.randrange(1, 40))) for _ in range(n)]


def small_vocab():
    keys = ["[UNK]", "[CLS]", "[SEP]"] + sorted(set(POOL) - set(" \t\n\r\x00")) + ["##" + c for c in "abcxyz019éüαβбг한글"]
    keys += ["ab", "abc", "##bc", "##cx", "xyz", "##yz", "hello", "world", "caf", "##e", "naive", "한글", "##가"]
    return {k: i for i, k in enumerate(dict.fromkeys(keys))}


@pytest.mark.parametrize("lowercase,strip_accents", OPTS)
def test_table_agrees_with_reference(lowercase, strip_accents):
    for t in FIXED + draw(1, 500):
        assert wp.normalize_words(t, lowercase, strip_accents) == ref.words(t, lowercase, strip_accents), repr(t)


def test_table_agrees_without_cjk_and_clean_up():
    for t in FIXED + draw(2, 300):
        assert wp.normalize_words(t, True, None, False, False) == ref.words(t, True, None, False, False), repr(t)


@pytest.mark.parametrize("lowercase,strip_accents", OPTS)
def test_agrees_with_hugging_face(lowercase, strip_accents):
    tk = pytest.importorskip("tokenizers")
    vocab = small_vocab()
    hf = tk.Tokenizer(tk.models.WordPiece(vocab, unk_token="[UNK]", max_input_chars_per_word=100))
    hf.normalizer = tk.normalizers.BertNormalizer(clean_text=True, handle_chinese_chars=True, strip_accents=strip_accents, lowercase=lowercase)
    hf.pre_tokenizer = tk.pre_tokenizers.BertPreTokenizer()
    for t in FIXED + draw(3, 1500):
        want = hf.encode(t, add_special_tokens=False).ids
        assert ref.encode(t, vocab, vocab["[UNK]"], lowercase=lowercase, strip_accents=strip_accents) == want, repr(t)
        got = [i for w in wp.normalize_words(t, lowercase, strip_accents) for i in ref.encode_word(w, vocab, vocab["[UNK]"])]
        assert got == want, repr(t)


def test_table_builder_facts():
    """build_norm_table asserts them for every code point; here they are read back from the finished tables."""
    for lowercase, strip_accents in OPTS:
        table = wp.build_norm_table(lowercase, strip_accents)
        for c in list(range(0x0600)) + [0x1E9B, 0x1F82, 0x2126, 0x3000, 0x4E00, 0xF900, 0xAC01, 0xD7A3, 0xFB2C, 0x1D160, 0x1D164, 0x10FFFF]:
            out = wp.table_lookup(table, c)
            n_in, n_out = len(chr(c).encode("utf-8", "surrogatepass")), sum(len(chr(o).encode()) for o, _ in out)
            assert len(out) <= 3 and n_out - n_in <= 8 and len(out) <= n_in
            assert out == wp.map_code_point(c, lowercase, strip_accents, True, True)
    assert wp.table_lookup(wp.build_norm_table(), 0x1D160) == ((0x1D158, 0), (0x1D165, 0), (0x1D16E, 0))
    assert len(wp.table_lookup(wp.build_norm_table(False, False), 0xAC01)) == 1 and len(wp.table_lookup(wp.build_norm_table(), 0xAC01)) == 3


@pytest.mark.parametrize("data,what", [(b"a\n\nb\n", "empty"), (b"a\nb\na\n", "twice"), (b"a\n" + b"x" * 256 + b"\n", "255"), (b"", "empty")])
def test_vocab_txt_refusals(data, what):
    with pytest.raises(ValueError, match="WordPiece mode.*" + what):
        wp.parse_vocab_txt(data)


def test_vocab_txt_lines():
    assert wp.parse_vocab_txt(b"[UNK]\r\n##a\nb") == [b"[UNK]", b"##a", b"b"]
