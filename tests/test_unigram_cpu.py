"""Unigram mode off the GPU: the plain reference (unigram_ref.py) against Hugging Face's tokenizers where that module imports, and
the definition's hand cases.  (A handle cannot be made without a GPU: the create-time refusals are in test_gpu_unigram.py.)"""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import unigram_ref as ref  # noqa: E402

# exact ties (multiples of 0.5), no key for z alone, multi-byte keys, a key with a tab
PIECES = [("<unk>", 0.0), ("▁", -2.0), ("a", -3.0), ("b", -3.5), ("ab", -6.5), ("c", -4.0), ("abc", -10.5), ("▁a", -5.0), ("▁ab", -8.5),
          ("é", -5.0), ("日", -5.5), ("本", -5.5), ("日本", -11.0), ("a\tb", -7.0), ("\t", -6.5), ("bc", -7.5), ("zé", -9.0), ("▁▁", -4.0)]
HAND = ["", " ", "a  b", "▁ab", "a▁b", "zqz ab", "日本日x"]


def draw(seed, n):
    rng = random.Random(seed)
    return ["".join(rng.choice("abc z é ▁ \t 日 本") for _ in range(rng.randrange(0, 24))) for _ in range(n)]


def test_definition_by_hand():
    P = [("<unk>", 0.0), ("a", -3.0), ("b", -3.5), ("ab", -6.5), ("▁", -1.0)]
    assert ref.encode("ab", P, 0, "never") == [3]             # the tie keeps the earliest start
    assert ref.encode("a  b", P, 0) == [4, 1, 4, 4, 2] and ref.words("a  b") == ["▁a", "▁", "▁b"]
    assert ref.encode("qqa q", P, 0, "never") == [0, 1, 4, 0] and ref.encode("", P, 0) == []      # a run of unk is one id
    assert ref.encode(b"a\xffb", P, 0, "never") == [1, 0, 2]


@pytest.mark.parametrize("prepend", ["always", "never"])
def test_agrees_with_hugging_face(prepend):
    tk = pytest.importorskip("tokenizers")
    hf = tk.Tokenizer(tk.models.Unigram([(p, s) for p, s in PIECES], unk_id=0, byte_fallback=False))
    hf.pre_tokenizer = tk.pre_tokenizers.Metaspace(replacement="▁", prepend_scheme=prepend)
    for t in HAND + draw(7, 3000):
        assert ref.encode(t, PIECES, 0, prepend) == hf.encode(t, add_special_tokens=False).ids, repr(t)
