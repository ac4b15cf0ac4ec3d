"""Unigram mode on the GPU (csrc/spl_k_uni.h), bit-exact against the plain reference (unigram_ref.py): through the C ABI
(spl_encode_batch_device on raw bytes) and through Tokenizer.  The tile is 512 bytes, the halo 128 (UNI_TB, UNI_H)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import unigram_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
TB, H = 512, 128

# exact ties everywhere (multiples of 0.5): ab = a + b, 日本 = 日 + 本, xx = x + x, every a^k = k * a; no key for q; a key with a tab
PIECES = [("<unk>", 0.0), ("<s>", 0.0), ("</s>", 0.0), ("<pad>", 0.0), ("▁", -2.0), ("b", -3.5), ("ab", -6.5), ("c", -4.0), ("▁a", -4.5),
          ("▁ab", -8.0), ("é", -5.0), ("日", -5.5), ("本", -5.5), ("日本", -11.0), ("a\tb", -7.0), ("\t", -6.5), ("x", -6.0), ("xx", -12.0),
          ("z", -7.5), ("bc", -7.0), ("▁日", -8.0), ("cé", -8.5)] + [("a" * k, -3.0 * k) for k in range(1, 17)]
UNK = 0


@pytest.fixture(scope="module", params=["always", "never"])
def tok(request):
    from splintr_amd import Tokenizer
    t = Tokenizer.from_bytes_unigram(PIECES, UNK, prepend_scheme=request.param)
    t.scheme = request.param
    return t


def want(tok, doc):
    return ref.encode(doc, PIECES, UNK, tok.scheme)


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


def filler(n):
    return ("ab c " * (n // 5 + 1))[:n]


def at_tile_edge(word):
    """Documents, each a whole number of tiles, with `word` at every offset -3 .. +3 around a tile boundary."""
    docs = []
    for d in range(-3, 4):
        doc = filler(TB + d) + word
        docs.append(doc + filler(-len(doc.encode()) % TB))
    return docs


CASES = {
    "hand": ["", " ", "a  b", "▁ab", "a▁b", "zqz ab", "日本日x", "ab", "a\tb a\tc", "qq▁q q", "▁", "  ", "xxx xx"],
    "empty_documents": ["", "", "ab c", "", "", " a", "b", "", ""],
    "invalid_utf8": [b"ab\xffcd \xe2\x96 x\xc3", b"\x81\xa9ab", b"a\xe2\x96", b"\x96\x81b \xe6\x97\xa5\xe6\x97"],
    "edge_space": at_tile_edge(" 日本é ab"),
    "edge_literal_marker": at_tile_edge("▁ab▁日本céz"),
    "edge_multibyte": at_tile_edge("日本日本é日 ▁"),
    "halo_lengths": [s + "a" * (n - 1) + " ab" for n in (H - 1, H, H + 1) for s in ("ab ", "▁")] + ["xx" * (H // 2) + " b", "x" * (H + 1)],
    "long_words": ["ab " + "a" * (5 * TB) + " ab", "q" * (5 * TB), "c " + "é" * 700 + "ab" + "日本" * 300 + " c", "b" * 1000 + "q" * 70 + "b" * 90],
    "dense_pool_overflow": ["aaaaaaaaaaaaaaaaaaaa " * 100, ("a" * 100 + " ") * 12],
    "thousand_docs": [("ab cé q日本 " * (i % 7))[: i % 23] for i in range(1000)],
}


@pytest.mark.parametrize("case", list(CASES))
def test_device_call(tok, case):
    docs = CASES[case]
    got, need = device_encode(tok, docs)
    assert got == [want(tok, d) for d in docs]
    assert need == sum(map(len, got))


@pytest.mark.parametrize("docs", [["ab c", filler(700), "a" * 200 + " b"], ["b"] * 300], ids=["mixed", "need_beyond_n_bytes"])
def test_capacity_one_short(tok, docs):
    full = [want(tok, d) for d in docs]
    got, need = device_encode(tok, docs, short=1)
    assert need == sum(map(len, full)) and got == full[:-1] + [full[-1][:-1]]
    if tok.scheme == "always" and docs[0] == "b":
        assert need == 2 * len(docs)                        # more ids than bytes: the prepended marker is a token of its own


def _create(flags, keys, scores, unk_id=0, pattern=0):
    from splintr_amd import _ffi, tokenizer
    blob = "".join(k + "\n" for k in keys).encode()
    ucls = tokenizer._read(tokenizer._unicode_table_path("pcre2"))
    arr = (ctypes.c_double * len(scores))(*scores)
    opts = _ffi.SplOpts(pattern, 0, flags, b"a+" if pattern else None, unk_id=unk_id, scores=arr, uni_flags=1)
    h = _ffi.lib().spl_create(blob, len(blob), ucls, len(ucls), ctypes.byref(opts))
    return h, _ffi.last_error()


@pytest.mark.parametrize("flags,keys,scores,pattern,what", [
    (16 | 1, ["u", "a"], [0.0, -1.0], 0, "SPL_OPT_BYTE_LEVEL"), (16 | 2, ["u", "a"], [0.0, -1.0], 0, "SPL_OPT_SENTENCEPIECE"),
    (16 | 4, ["u", "a"], [0.0, -1.0], 0, "SPL_OPT_KEEP_ALL_IDS"), (16 | 8, ["u", "a"], [0.0, -1.0], 0, "SPL_OPT_WORDPIECE"),
    (16, ["u", "a"], [0.0, -1.0], 3, "custom pattern"), (16, ["u", "a"], [0.0], 0, "n_scores"), (16, ["u", "a"], [10.0, 11.0], 0, "min_score - 10"),
    (16, ["u", "a", "a"], [0.0, -1.0, -1.0], 0, "twice"), (16, ["u", "", "a"], [0.0, -1.0, -1.0], 0, "empty line"),
    (16, ["u", "a" * 256], [0.0, -1.0], 0, "255"), (16, ["u", "a"], [0.0, float("inf")], 0, "not finite")])
def test_create_refusals(flags, keys, scores, pattern, what):
    h, err = _create(flags, keys, scores, pattern=pattern)
    assert not h and "Unigram mode" in err and what in err, err


def test_call_refusals():
    from splintr_amd import Tokenizer, _ffi
    t = Tokenizer.from_bytes_unigram(PIECES, UNK, special_tokens={"<s>": 1})
    with pytest.raises(Exception, match="Unigram mode.*SPL_WITH_SPECIAL"):
        t.encode_batch_with_special(["ab"])
    z = torch.zeros(64, dtype=torch.int64, device="cuda")
    rc = _ffi.lib().spl_encode_chunks_device(t.handle, z.data_ptr(), 0, z.data_ptr(), 1, z.data_ptr(), z.data_ptr(), z.data_ptr(), 0, z.data_ptr(), None)
    assert rc != 0 and "Unigram mode" in _ffi.last_error()


def test_tokenizer_methods(tok, tmp_path):
    from splintr_amd import Tokenizer
    texts = ["ab c日本", "", "zqz  ab", filler(1300) + "a" * 300]
    assert tok.is_unigram() and not tok.is_wordpiece() and tok.encode_batch(texts) == [want(tok, t) for t in texts]
    assert tok.encode("a\tb ab") == want(tok, "a\tb ab")
    assert tok.decode(want(tok, "ab  c日本")) == "ab  c日本" and tok.decode_batch([want(tok, " ab")]) == [" ab" if tok.scheme == "never" else "ab"]
    cfg = {"normalizer": {"type": "NFKC"}, "pre_tokenizer": {"type": "Metaspace", "replacement": "▁", "prepend_scheme": tok.scheme},
           "model": {"type": "Unigram", "unk_id": UNK, "vocab": [list(p) for p in PIECES]}, "added_tokens": [{"id": 1, "content": "<s>", "special": True}]}
    path = tmp_path / "tokenizer.json"
    path.write_text(json.dumps(cfg), encoding="utf-8")
    with pytest.raises(ValueError, match="NFKC"):
        Tokenizer.from_tokenizer_json(str(path))
    assert Tokenizer.from_tokenizer_json(str(path), ignore_normalizer=True).encode_batch(texts) == [want(tok, t) for t in texts]
    cfg["model"]["type"] = "BPE"
    path.write_text(json.dumps(cfg), encoding="utf-8")
    with pytest.raises(ValueError, match="BPE"):
        Tokenizer.from_tokenizer_json(str(path), ignore_normalizer=True)


def test_pairs_end_to_end(tok):
    a, b = ["ab c", "zqz"], ["日本 x", "a" * 20 + " b"]
    bos, eos, pad, n = 1, 2, 3, 32
    out = tok.encode_batch_pairs(a, b, n, pad_id=pad, prefix=[bos], middle=[eos, eos], suffix=[eos])
    for i in range(2):
        row = [bos] + want(tok, a[i]) + [eos, eos] + want(tok, b[i]) + [eos]
        assert out[0][i].tolist() == row + [pad] * (n - len(row)) and int(out[4][i]) == len(row)
