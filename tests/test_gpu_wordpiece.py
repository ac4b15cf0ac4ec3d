"""WordPiece mode on the GPU (csrc/spl_k_wp.h), bit-exact against the plain reference (wordpiece_ref.py): through the C ABI
(spl_encode_batch_device on raw bytes) and through Tokenizer (encode_batch, encode_batch_pairs)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import wordpiece_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# (lowercase, strip_accents, max_input_chars_per_word): the default, nothing folded, and a word limit that makes its edge cheap
OPTS = [(True, None, 100), (False, False, 100), (True, None, 4)]
SINGLE = "abcdefghijklmnoprstuvwxyzABCXéèüeαβγσςбгджあア中文漢한글가각\u0301!#.,;-()$+§«»…0123456789"       # (no q)


def vocab_keys():
    keys = ["[PAD]", "[UNK]", "[CLS]", "[SEP]"] + list(dict.fromkeys(SINGLE)) + ["##" + c for c in dict.fromkeys(SINGLE) if c not in "!#.,;-()$+§«»…中文漢"]
    keys += ["ab", "abcd", "##cx", "xy", "##yq", "xq", "hello", "world", "##ld", "caf", "cafe", "##é", "한글", "##글한", "αβ", "##γ", "бг", "aaaa", "##aaa",
             "##", "#a", "the", "##ing", "token", "##izer", "##s"]
    return list(dict.fromkeys(keys))


KEYS = vocab_keys()
VOCAB = {k: i for i, k in enumerate(KEYS)}
UNK = VOCAB["[UNK]"]


@pytest.fixture(scope="module", params=OPTS, ids=lambda o: f"lc{int(o[0])}-sa{o[1]}-max{o[2]}")
def tok(request):
    from splintr_amd import Tokenizer
    lc, sa, mx = request.param
    t = Tokenizer.from_bytes_wordpiece("\n".join(KEYS).encode() + b"\n", lowercase=lc, strip_accents=sa, max_input_chars_per_word=mx)
    t.opts = request.param
    return t


def want(tok, doc):
    lc, sa, mx = tok.opts
    return ref.encode(doc, VOCAB, UNK, mx, "##", lowercase=lc, strip_accents=sa)


def device_encode(tok, docs, short=0):
    """spl_encode_batch_device on raw bytes: (ids per document, the need the call reports); `short` ids fewer than the need of room."""
    from splintr_amd import _ffi
    docs = [d.encode() if isinstance(d, str) else d for d in docs]
    buf = b"".join(docs)
    off = np.cumsum([0] + [len(d) for d in docs]).astype(np.int64)
    text = torch.from_numpy(np.frombuffer(buf + b"\0" * ((-len(buf)) % 16 + 16), dtype=np.uint8).copy()).cuda()
    d_off, out_off = torch.from_numpy(off).cuda(), torch.full((len(docs) + 1,), -1, dtype=torch.int64, device="cuda")
    need = sum(len(want(tok, d)) for d in docs)
    cap = max(need - short, 0)
    ids = torch.full((cap + 8,), -7, dtype=torch.int32, device="cuda")
    rc = _ffi.lib().spl_encode_batch_device(tok.handle, text.data_ptr(), len(buf), d_off.data_ptr(), len(docs), 0, ids.data_ptr(), cap,
                                            out_off.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _ffi.last_error()
    oo, flat = out_off.cpu().tolist(), ids.cpu().tolist()
    assert flat[cap:] == [-7] * 8, "ids written beyond ids_capacity"
    return [flat[oo[i]:min(oo[i + 1], cap)] for i in range(len(docs))], oo[-1]


LONG = ("hello world abcx xyq xqz cafe\u0301 Café naïve αβγ Σσς бгд ab中文cd tokenizers, the-tokening!! "
        "한글한글한 a\xadb x\u200by $5+3 «ab»… #a a# ## aaaaaaa あア qab abq ") * 55           # ~10 KB: three normaliser tiles, five and more of the matcher's
CASES = {
    "abcx": ["abcx", "abcd abc ab a"],
    "greedy_dead_is_unk": ["xyq"],                                  # xy, then no ##q: unk although x ##yq exists
    "unreached_dead_is_fine": ["xqz", "xqs"],                       # q has no key of its own, but the walk never lands on it
    "hash_keys": ["#a", "a#", "##", "a##a #a#"],
    "word_limit": ["a" * 99, "a" * 100, "a" * 101, "abcd abcde", "é" * 100 + " " + "é" * 101, "a" * 7000 + " ab"],
    "empty_and_dropped": ["", " ", "   \t\n", "\x00\u200b\ufeff", "", "ab", "cd", "", "\u200b", "a\u200b", "\u200bb", " ", ""],
    "scripts": ["café cafe\u0301 CAFÉ", "αβγ ΑΒΓ σς", "бгДЖ", "ab中文cd漢", "!!..,;-(a)", "a\xadb",
                "한글가 각", "\u037e a\u037eb"],
    "hangul_at_tile_edge": [" " * 4090 + "한글한글한글 ab", "a " * 680 + "한글" * 30],
    "invalid_utf8": [b"ab\xffcd \xe2\x82 x\xc0\x80y \xed\xa0\x80z \xf4\x90\x80\x80 \xf0\x9f\x98", b"a\xe2\x82", b"\xacb", b"\x80\x80ab\xe2"],
    "thousand_docs": [("ab cd xyq " * (i % 7))[: i % 23] for i in range(1000)],
}


@pytest.mark.parametrize("case", list(CASES))
def test_device_call(tok, case):
    docs = CASES[case]
    got, need = device_encode(tok, docs)
    assert got == [want(tok, d) for d in docs]
    assert need == sum(map(len, got))


@pytest.mark.parametrize("shift", range(17))
def test_tile_edges(tok, shift):
    """Every word of a text of several tiles meets the normaliser's and the matcher's tile edges at some shift."""
    doc = "z" * shift + LONG
    got, _ = device_encode(tok, [doc])
    assert got == [want(tok, doc)]


def test_capacity_one_short(tok):
    docs = ["hello world", LONG[:300], "abcx"]
    full = [want(tok, d) for d in docs]
    got, need = device_encode(tok, docs, short=1)
    assert need == sum(map(len, full)) and got == [full[0], full[1], full[2][:-1]]


def test_tokenizer_methods(tok):
    texts = ["hello world", "", "abcx xyq", LONG[:500]]
    assert tok.is_wordpiece() and tok.encode_batch(texts) == [want(tok, t) for t in texts]
    assert tok.encode("Café abcx") == want(tok, "Café abcx")
    assert tok.decode_bytes(want(tok, "abcx")) == b"ab##cx"
    with pytest.raises(NotImplementedError, match="WordPiece"):
        tok.decode([1])


def test_pairs_end_to_end(tok):
    a, b = ["hello world", "abcx"], ["the tokenizers", "xyq xqz café"]
    cls, sep, pad, n = VOCAB["[CLS]"], VOCAB["[SEP]"], VOCAB["[PAD]"], 24
    out = tok.encode_batch_pairs(a, b, n, pad_id=pad, prefix=[cls], middle=[sep], suffix=[sep])
    for i in range(2):
        row = [cls] + want(tok, a[i]) + [sep] + want(tok, b[i]) + [sep]
        types = [0] * (len(want(tok, a[i])) + 2) + [1] * (len(want(tok, b[i])) + 1)
        assert out[0][i].tolist() == row + [pad] * (n - len(row))
        assert out[2][i].tolist()[: len(row)] == types and int(out[4][i]) == len(row)
