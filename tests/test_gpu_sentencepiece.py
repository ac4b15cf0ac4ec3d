"""GPU tests (-m gpu) of SentencePiece mode (csrc/spl_k_sp.h): device ids against the restated reference loop (tests/sp_ref.py) through
encode, encode_batch and encode_batch_with_special, with the one-launch form and the chunk memo each on and off; the two ways a
duplicated key loads; decode; and the caller's-buffer contract of spl_encode_batch_device on this path."""
import base64
import ctypes
import itertools
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim"))
import sp_ref  # noqa: E402
from sp_sim import CASES, SPECIAL  # noqa: E402

pytestmark = pytest.mark.gpu

MARK = "▁".encode()
# the 256 single bytes; a lone half of the marker, the marker and what merges through it; a key of two newlines, which no chunk of the
# mode can ever be (every non-space byte of an ASCII-led whitespace run is a chunk of its own); one key listed twice
KEYS = [bytes([b]) for b in range(256)] + [MARK[:2], MARK, MARK * 2, MARK + b"a", b"ab", MARK + b"ab", b"\n\n", b"ba", b"ba"]
VOCAB = b"".join(base64.b64encode(k) + b" %d\n" % i for i, k in enumerate(KEYS))
NLNL, BA_FIRST, BA_LAST = 262, 263, 264
FIRST = {}
for _i, _k in enumerate(KEYS):
    FIRST.setdefault(_k, _i)
LAST = {k: i for i, k in enumerate(KEYS)}


@pytest.fixture(scope="module")
def toks():
    from splintr_amd import SENTENCEPIECE_PATTERN, Tokenizer
    return (Tokenizer.from_bytes_sentencepiece(VOCAB, SENTENCEPIECE_PATTERN, SPECIAL),
            Tokenizer.from_bytes_sentencepiece_with_decoder(VOCAB, SENTENCEPIECE_PATTERN, SPECIAL))


def _opt(t, name, v):
    from splintr_amd import _ffi
    assert _ffi.lib().spl_set_option(t.handle, name, v) == 0, _ffi.last_error()


@pytest.mark.parametrize("fuse,memo", itertools.product((1, 0), (1, 0)))
@pytest.mark.parametrize("name", sorted(CASES))
def test_ids_match_reference(toks, name, fuse, memo):
    t, texts = toks[0], CASES[name]
    _opt(t, b"fuse", fuse)
    _opt(t, b"memo", memo)
    try:
        want = [sp_ref.encode(x, LAST) for x in texts]
        assert t.encode_batch(texts) == want
        assert t.encode(texts[0]) == want[0]
        got = t.encode_batch_with_special(texts)
        assert got == [sp_ref.encode_with_special(x, LAST, SPECIAL) for x in texts]
        assert all(NLNL not in ids for ids in got)
    finally:
        _opt(t, b"fuse", 1)
        _opt(t, b"memo", 1)


def test_duplicated_key_and_decode(toks):
    plain, keep = toks
    assert plain.encode("ba") == [BA_LAST] and keep.encode("ba") == [BA_FIRST]
    assert keep.encode("ab ba") == sp_ref.encode("ab ba", FIRST)
    assert keep.decode([BA_FIRST, BA_LAST]) == "baba" and plain.decode([BA_FIRST, BA_LAST]) == "ba"
    assert keep.decode_bytes(keep.encode(" a")) == MARK + b"a"          # (the vocabulary's own bytes)
    for texts in CASES.values():
        for s in texts:
            if "▁" not in s:
                assert plain.decode(plain.encode(s)) == s
    assert plain.decode_batch([plain.encode(" ab  a")]) == [" ab  a"] and plain.decode_lossy([0xE2]) == "�"


@pytest.mark.parametrize("cap_less", [1, 40])
def test_device_call_capacity_and_footprint(toks, cap_less):
    """spl_encode_batch_device with ids_capacity below the need: the offsets are complete, the ids are the result's first entries,
    nothing is stored at or beyond the capacity."""
    import numpy as np
    import torch
    from splintr_amd import _ffi
    t = toks[0]
    texts = CASES["three_tiles"] + CASES["space_newline_spaces"]
    want = [sp_ref.encode(x, LAST) for x in texts]
    flat = [i for w in want for i in w]
    raw = b"".join(x.encode() for x in texts)
    dev = torch.device("cuda", 0)
    text = torch.frombuffer(bytearray(raw + b"  ab" * 8), dtype=torch.uint8).to(dev)
    off = torch.from_numpy(np.cumsum([0] + [len(x.encode()) for x in texts]).astype(np.int64)).to(dev)
    cap = len(flat) - cap_less
    ids = torch.full((len(flat) + 64,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    out_off = torch.zeros(len(texts) + 1, dtype=torch.int64, device=dev)
    rc = _ffi.lib().spl_encode_batch_device(ctypes.c_void_p(t.handle), ctypes.c_void_p(text.data_ptr()), ctypes.c_uint64(len(raw)),
                                            ctypes.c_void_p(off.data_ptr()), ctypes.c_uint64(len(texts)), ctypes.c_uint32(0),
                                            ctypes.c_void_p(ids.data_ptr()), ctypes.c_uint64(cap), ctypes.c_void_p(out_off.data_ptr()),
                                            ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0, _ffi.last_error()
    torch.cuda.synchronize(dev)
    assert out_off.tolist() == np.cumsum([0] + [len(w) for w in want]).tolist()
    got = ids.tolist()
    assert got[:cap] == flat[:cap] and set(got[cap:]) == {0x5A5A5A5A}
