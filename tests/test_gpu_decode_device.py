"""GPU tests (-m gpu) of spl_decode_batch_device (csrc/spl_k_decode_dev.h): ids in HBM -- a CSR, or rows with a validity predicate -- to a
bytes CSR in HBM.

Expected bytes: oracle/pyoracle.py's decode_bytes per document (SKIP_SPECIAL applied here from o.special_tokens / o.encoder; clamping,
row validity and the capacity cut applied here as the header states them).  Every output lies in an allocation 64 bytes (one offset)
longer than the capacity, filled with 0xA5: each check asserts that everything at or beyond min(need, capacity) still holds it.
Shapes are the smallest at which each mechanism can go wrong: id counts around the 1 024-slot block, byte counts around the 16-byte
group; the mapping itself is tested exhaustively on the CPU (tests/test_decode_device_cpu.py)."""
import ctypes
import os
import random

import numpy as np
import pytest

import vocabgen
from conftest import ROOT
from decode_ref import I64, PAD_LEFT, SKIP_SPECIAL
from fuzzgen import fuzz_corpus
from test_gpu_decode import pair

pytestmark = pytest.mark.gpu

TAIL = 64
POISON = 0xA5
OFF_POISON = -0x5A5A5A5A5A5A5A5B          # 0xA5A5... as int64
_made = {}


def _dev():
    import torch
    return torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------ tokenizers and what they decode to
def _lengths_pair():
    """the `lengths` family of tests/vocabgen.py: keys up to 300 bytes, sparse ids up to 2^21 - 2"""
    if "lengths" not in _made:
        from oracle.pyoracle import Oracle
        from splintr_amd import Tokenizer, CL100K_BASE_PATTERN
        enc = vocabgen.family("lengths")[0]
        _made["lengths"] = (Tokenizer.from_bytes(vocabgen.tiktoken(enc), CL100K_BASE_PATTERN), Oracle(enc, CL100K_BASE_PATTERN, False))
    return _made["lengths"]


FAR = {"<|far|>": 2 ** 31 - 1, "<|mid|>": 5_000_000, "<|near|>": 100300, "<|" + "L" * 251 + "|>": 100301}


def _far_pair():
    """cl100k_base with specials at 100300, 100301 (a 255-byte literal), 5 000 000 and 2^31 - 1"""
    if "far" not in _made:
        from oracle import pyoracle as O
        from splintr_amd import Tokenizer, CL100K_BASE_PATTERN
        path = os.path.join(ROOT, "splintr_amd", "data", "cl100k_base.splv")
        with open(path, "rb") as f:
            blob = f.read()
        _made["far"] = (Tokenizer.from_bytes(blob, CL100K_BASE_PATTERN, FAR), O.Oracle(O.load_splv(path)[0], CL100K_BASE_PATTERN, False, FAR))
    return _made["far"]


def _pair(name):
    return {"lengths": _lengths_pair, "far": _far_pair}.get(name, lambda: pair(name))()


def _special_only(o):
    return set(o.special_tokens.values()) - set(o.encoder.values())


def _doc_bytes(o, ids, flags):
    """one document's bytes: ids is a list of Python ints (int64 values may be negative or beyond 32 bits: no ids)"""
    ids = [int(i) if flags & I64 else int(i) & 0xFFFFFFFF for i in ids]
    ids = [i for i in ids if 0 <= i < 2 ** 32]
    if flags & SKIP_SPECIAL:
        so = _special_only(o)
        ids = [i for i in ids if i not in so]
    return o.decode_bytes(ids)


def _finish(docs):
    off = [0]
    for d in docs:
        off.append(off[-1] + len(d))
    return b"".join(docs), off


def _want_csr(o, ids, off, n_cap, flags=0):
    c = [min(int(x), int(n_cap)) for x in off]
    return _finish([_doc_bytes(o, ids[c[d]:c[d + 1]].tolist(), flags) for d in range(len(c) - 1)])


def _want_rows(o, rows, lens, flags):
    n, L = rows.shape
    docs = []
    for r in range(n):
        k = L if lens is None else max(0, min(int(lens[r]), L))
        docs.append(_doc_bytes(o, (rows[r, L - k:] if flags & PAD_LEFT else rows[r, :k]).tolist(), flags))
    return _finish(docs)


def _by_length(o, n_max=40):
    """length -> an id of the vocabulary that decodes to that many bytes"""
    key = ("bylen", id(o))
    if key not in _made:
        m = {}
        for k, i in o.encoder.items():
            n = len(o.decode_bytes([i]))
            if n <= n_max and n not in m:
                m[n] = i
        _made[key] = m
    return _made[key]


def _mixed_ids(o, rng, n, p_unknown=0.2):
    """n ids: vocabulary ids of all kinds, specials, and ids of neither map (holes, beyond every table)"""
    top = max(o.encoder.values())
    sp = sorted(o.special_tokens.values()) or [top + 7]
    known = set(o.encoder.values()) | set(sp)
    out = np.empty(n, dtype=np.uint32)
    for i in range(n):
        r = rng.random()
        if r < p_unknown:
            out[i] = rng.choice([x for x in (top + 1, top + 5000, 2 ** 31 - 2, 2 ** 32 - 1, 4_999_999) if x not in known])
        elif r < p_unknown + 0.1:
            out[i] = rng.choice(sp)
        else:
            out[i] = rng.randrange(min(top + 1, 300)) if rng.random() < 0.1 else rng.randrange(top + 1)
    return out


# ------------------------------------------------------------------------------------------ one call into guarded buffers
def _call(t, ids, n_cap, off, lens, n_docs, flags, row_len, capacity, null_bytes=False):
    """ids: a numpy array (uint32 / int32 / int64, any shape); off / lens: numpy or None -> (bytes below min(need, capacity), offsets)"""
    import torch
    from splintr_amd import _ffi
    dev = _dev()
    ids = np.ascontiguousarray(ids)
    if ids.dtype == np.uint32:
        ids = ids.view(np.int32)
    d_ids = torch.from_numpy(np.concatenate([ids.reshape(-1), np.zeros(4, ids.dtype)])).to(dev)           # (never a null pointer)
    d_off = None if off is None else torch.from_numpy(np.asarray(off).astype(np.int64)).to(dev)
    d_len = None if lens is None else torch.from_numpy(np.asarray(lens).astype(np.int32)).to(dev)
    out = torch.full((capacity + TAIL,), POISON, dtype=torch.uint8, device=dev)
    out_off = torch.full((n_docs + 2,), OFF_POISON, dtype=torch.int64, device=dev)
    o = _ffi.SplDecodeOpts(flags, row_len)
    rc = _ffi.lib().spl_decode_batch_device(t.handle, d_ids.data_ptr(), n_cap, None if d_off is None else d_off.data_ptr(),
                                            None if d_len is None else d_len.data_ptr(), n_docs, ctypes.byref(o),
                                            None if null_bytes else out.data_ptr(), capacity, out_off.data_ptr(),
                                            torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, _ffi.last_error()
    oo = out_off.cpu().numpy()
    assert oo[-1] == OFF_POISON, "written behind the offsets"
    need = int(oo[n_docs])
    raw = out.cpu().numpy()
    m = min(need, capacity)
    assert (raw[m:] == POISON).all(), "written at or beyond min(need, capacity)"
    return raw[:m].tobytes(), oo[:-1].tolist()


def _check_csr(name, ids, off, tag, *, n_cap=None, flags=0, capacity=None, poison_tail=0, null_bytes=False):
    t, o = _pair(name)
    ids = np.asarray(ids)
    off = np.asarray(off, dtype=np.uint64)
    if poison_tail:                                       # ids behind the CSR's end that WOULD decode to something
        ids = np.concatenate([ids, np.full(poison_tail, _by_length(o)[3], dtype=ids.dtype)])
    n_cap = len(ids) if n_cap is None else n_cap
    w_raw, w_off = _want_csr(o, ids, off, n_cap, flags)
    cap = len(w_raw) if capacity is None else capacity
    raw, oo = _call(t, ids, n_cap, off, None, len(off) - 1, flags, 0, cap, null_bytes)
    assert oo == w_off, tag
    assert raw == w_raw[:cap], tag
    return len(w_raw)


def _split(rng, n, n_docs):
    cuts = sorted(rng.randrange(n + 1) for _ in range(max(n_docs - 1, 0)))
    return np.array([0] + cuts + [n], dtype=np.uint64) if n_docs else np.zeros(1, dtype=np.uint64)


# ------------------------------------------------------------------------------------------ block edges
@pytest.mark.parametrize("name", ["cl100k_base", "deepseek_v3"])
def test_block_edges(name):
    t, o = _pair(name)
    rng = random.Random(11)
    for n in (0, 1, 1023, 1024, 1025, 2048, 2049, 3073):
        ids = _mixed_ids(o, rng, n)
        if n > 3:
            ids[:3] = [0, 1, 2]                           # (deepseek: keys that are not ByteLevel text)
        _check_csr(name, ids, [0, n], (name, n, "one document"))
        _check_csr(name, ids, _split(rng, n, 7), (name, n, "seven documents"), flags=SKIP_SPECIAL)
    # block sums of chosen residues: the first block's byte count is 1, 2, 3 (mod 4) and 1, 15 (mod 16) -- its range ends one byte into a
    # 16-byte group, or one byte short of one, and the next block's starts there.  Four-byte tokens, ONE token of n_odd bytes and k unknown ids
    # (in front of tokens), k chosen so that 4 * (1023 - k) + n_odd has the wanted residue; asserted from the oracle.
    by = _by_length(o)
    for n_odd, want16 in ((1, 1), (15, 15), (17, 1), (2, 2), (3, 3), (3, 15), (1, 13)):
        k = next(k for k in range(1, 6) if (4 * (1023 - k) + n_odd) % 16 == want16)
        ids = np.full(2049, by[4], dtype=np.uint32)
        ids[5] = by[n_odd]
        ids[[700, 300, 900, 100, 500][:k]] = 2 ** 32 - 1
        block_sum = len(o.decode_bytes(ids[:1024].tolist()))
        assert block_sum % 16 == want16 and block_sum % 4 == n_odd % 4 != 0, (name, n_odd, want16, block_sum)
        need = _check_csr(name, ids, [0, 5, 2049], (name, "residue", n_odd, want16))
        assert need == (2048 - k) * 4 + n_odd
    # a block of 1 024 unknown ids (zero bytes) between two ordinary blocks, first, and last
    unk = np.full(1024, 2 ** 31 - 2, dtype=np.uint32)
    for parts in ([_mixed_ids(o, rng, 1024), unk, _mixed_ids(o, rng, 700)], [unk, _mixed_ids(o, rng, 1025)], [_mixed_ids(o, rng, 1024), unk]):
        ids = np.concatenate(parts)
        _check_csr(name, ids, _split(rng, len(ids), 5), (name, "zero block", len(parts)))


def test_long_tokens():
    t, o = _pair("lengths")
    long_id = next(i for k, i in o.encoder.items() if len(k) == 300)
    need = _check_csr("lengths", np.full(1100, long_id, dtype=np.uint32), [0, 1, 1024, 1100], "300-byte key")        # one block: 307 200 bytes
    assert need == 330000
    rng = random.Random(5)
    known = sorted(o.encoder.values())
    ids = np.array([rng.choice(known) for _ in range(2500)] + [2 ** 21 - 2, 2 ** 21 - 1, 2 ** 21], dtype=np.uint32)
    _check_csr("lengths", ids, _split(rng, len(ids), 9), "sparse ids up to 2^21 - 2")
    singles = np.array([o.encoder[bytes([b])] for b in range(256)] * 5, dtype=np.uint32)
    assert _check_csr("lengths", singles, _split(rng, len(singles), 4), "single-byte tokens only") == 1280
    # a 255-byte special literal
    tf, of = _pair("far")
    ids = np.array([100301, 9906, 100301, 100301, 2 ** 31 - 1, 11], dtype=np.uint32)
    assert _check_csr("far", ids, [0, 2, 6], "255-byte literal") == 3 * 255 + 5 + 7 + 1
    assert _check_csr("far", ids, [0, 2, 6], "255-byte literal, skipped", flags=SKIP_SPECIAL) == 6
    from splintr_amd import _ffi
    assert _ffi.lib().spl_max_token_bytes(t.handle) == 300 and _ffi.lib().spl_max_token_bytes(tf.handle) == 255


def test_documents():
    name = "cl100k_base"
    t, o = _pair(name)
    rng = random.Random(12)
    z = np.zeros(0, dtype=np.uint32)
    _check_csr(name, z, [0], "n_docs = 0")
    _check_csr(name, z, [0, 0, 0, 0], "three empty documents and no id")
    ids = _mixed_ids(o, rng, 2500)
    for tag, off in (("5 000 empty first", [0] * 5000 + [1024, 2500]), ("5 000 empty at a block boundary", [0, 1024] + [1024] * 5000 + [2500]),
                     ("5 000 empty last", [0, 1000] + [2500] * 5000), ("one document over three blocks", [0, 10, 2300, 2500]),
                     ("a boundary exactly at slot 1 024", [0, 1024, 2500])):
        _check_csr(name, ids, off, tag)
    _check_csr(name, _mixed_ids(o, rng, 3000), np.arange(3001), "3 000 one-id documents")


def test_n_ids_cap_bounds_and_clamps():
    name = "cl100k_base"
    t, o = _pair(name)
    rng = random.Random(13)
    ids = _mixed_ids(o, rng, 2048, p_unknown=0.05)
    off = _split(rng, 2048, 40)
    _check_csr(name, ids, off, "the cap equals the count, a multiple of 1 024")
    _check_csr(name, ids[:1500], _split(rng, 1500, 9), "the cap equals the count")
    _check_csr(name, ids, off, "the cap far above the count", poison_tail=40000)
    for n_cap in (2047, 1025, 1024, 1, 0):                # the clamp: later documents' offsets equal the total; the ids beyond would decode
        _check_csr(name, ids, off, ("clamp", n_cap), n_cap=n_cap)


def test_capacity_cuts_the_bytes_never_the_offsets():
    name = "cl100k_base"
    t, o = _pair(name)
    rng = random.Random(14)
    ids = _mixed_ids(o, rng, 1500, p_unknown=0.1)
    off = _split(rng, 1500, 6)
    need = _check_csr(name, ids, off, "capacity = need")
    for cap in (need - 1, need - 15, need // 2, need // 2 + 7, 1029, 17, 16, 1):
        _check_csr(name, ids, off, ("capacity", cap), capacity=cap)
    _check_csr(name, ids, off, "capacity 0, d_bytes NULL", capacity=0, null_bytes=True)
    by = _by_length(o)
    ids = np.array([by[9]] * 10, dtype=np.uint32)         # 9-byte tokens: capacity 40 cuts token 4 in its middle and a group in its middle
    _check_csr(name, ids, [0, 10], "cut inside a token", capacity=40)


# ------------------------------------------------------------------------------------------ rows
@pytest.mark.parametrize("row_len", [1, 7, 1024, 1025])
def test_rows(row_len):
    t, o = _pair("far")
    rng = random.Random(row_len)
    n = {1: 2100, 7: 300, 1024: 3, 1025: 3}[row_len]
    rows = _mixed_ids(o, rng, n * row_len, p_unknown=0.1).astype(np.int64).reshape(n, row_len)      # padding slots hold ids that would decode
    rows.flat[::97] = 2 ** 31 - 1                                                                   # the far special
    lens = np.array([rng.randrange(-2, row_len + 3) for _ in range(n)], dtype=np.int32)
    lens[0], lens[n - 1], lens[n // 2] = 0, row_len, row_len + 100
    odd = rows.copy()
    odd.flat[::13] = [(-1, -100, 2 ** 32, 2 ** 32 + 17)[k & 3] for k in range(len(odd.flat[::13]))]
    r32 = rows.astype(np.uint32).view(np.int32)                                                     # int32 input is the 32-bit pattern
    for r, ln, flags in ((rows, None, I64), (rows, lens, I64), (rows, lens, I64 | PAD_LEFT), (odd, lens, I64 | PAD_LEFT | SKIP_SPECIAL),
                         (odd, None, I64), (r32, lens, 0), (r32, None, SKIP_SPECIAL), (r32, lens, PAD_LEFT)):
        w_raw, w_off = _want_rows(o, r, ln, flags)
        for cap in (len(w_raw), len(w_raw) // 2 + 3):
            raw, oo = _call(t, r, 0, None, ln, n, flags, row_len, cap)
            assert oo == w_off, (row_len, flags, cap)
            assert raw == w_raw[:cap], (row_len, flags, cap)
    # 2^32 + 17 must not alias id 17 (b"2"); without the flag the low word IS the id
    r = np.full((2, row_len), 2 ** 32 + 17, dtype=np.int64)
    assert _call(t, r, 0, None, None, 2, I64, row_len, 16)[0] == b""
    assert _call(t, np.full((2, row_len), 17, dtype=np.int64), 0, None, None, 2, I64, row_len, 2 * row_len)[0] == b"2" * (2 * row_len)


def _holes_pair():
    """the `lengths` vocabulary (sparse ids) with specials in a HOLE of the dense range, on a vocabulary id (both maps), and far away"""
    if "holes" not in _made:
        from oracle.pyoracle import Oracle
        from splintr_amd import Tokenizer, CL100K_BASE_PATTERN
        enc = vocabgen.family("lengths")[0]
        used = set(enc.values())
        hole = [i for i in range(1000, 3000) if i not in used][:3]
        both = enc[b"a"]
        sp = {"<|hole0|>": hole[0], "<|hole1|>": hole[1], "<|both|>": both, "<|far|>": 2 ** 31 - 1}
        _made["holes"] = (Tokenizer.from_bytes(vocabgen.tiktoken(enc), CL100K_BASE_PATTERN, sp), Oracle(enc, CL100K_BASE_PATTERN, False, sp), hole, both)
    return _made["holes"]


def test_skip_special():
    t, o, hole, both = _holes_pair()
    assert _special_only(o) == {hole[0], hole[1], 2 ** 31 - 1} and both in o.encoder.values()
    rng = random.Random(15)
    known = sorted(o.encoder.values())
    unit = [hole[0], both, known[3], hole[2], 2 ** 31 - 1, hole[1], both, 2 ** 31 - 2, known[40]]      # hole[2]: an id of neither map
    ids = np.array(unit * 250, dtype=np.uint32)
    off = _split(rng, len(ids), 11)
    for flags in (0, SKIP_SPECIAL):
        w_raw, w_off = _want_csr(o, ids, off, len(ids), flags)
        raw, oo = _call(t, ids, len(ids), off, None, 11, flags, 0, len(w_raw))
        assert oo == w_off and raw == w_raw, flags
    one = lambda f: _call(t, np.array(unit, dtype=np.uint32), len(unit), np.array([0, len(unit)]), None, 1, f, 0, 4096)[0]
    a, k3, k40 = b"a", o.decode_bytes([known[3]]), o.decode_bytes([known[40]])
    assert one(0) == b"<|hole0|>" + a + k3 + b"<|far|>" + b"<|hole1|>" + a + k40      # an id both maps hold is a vocabulary id
    assert one(SKIP_SPECIAL) == a + k3 + a + k40                                      # ... and is emitted
    # the far specials of a shipped vocabulary (every special of cl100k_base lies beyond its dense table)
    ids = np.array([9906, 100257, 11, 100300, 100301, 1917, 5_000_000, 2 ** 31 - 1, 0, 100262, 4_999_999] * 100, dtype=np.uint32)
    assert _check_csr("far", ids, _split(rng, len(ids), 5), "far specials skipped", flags=SKIP_SPECIAL) == 100 * len(b"Hello, world!")


# ------------------------------------------------------------------------------------------ round trips, no host copy in between
def _encode(t, texts):
    import torch
    from splintr_amd import device as dv
    batch = dv.DeviceBatch(texts, _dev())
    dv.encode_device(t, batch)
    return dv, batch


@pytest.mark.parametrize("which", ["fuzz", "c2"])
def test_encode_then_decode_gives_the_text_back(which):
    from splintr_amd import corpus
    t, o = _pair("cl100k_base")
    texts = fuzz_corpus(77, 300) + ["", ""] if which == "fuzz" else corpus.c2(1000)
    dv, batch = _encode(t, texts)
    out, off = dv.decode_device(t, batch.ids, batch.out_off, max_bytes=batch.n_bytes)        # n_ids_cap = ids.numel() = n_bytes: far above the count
    assert off.cpu().tolist() == batch.host_offsets.tolist()
    assert out[:batch.n_bytes].cpu().numpy().tobytes() == b"".join(x.encode("utf-8") for x in texts)
    assert out.numel() == (batch.n_bytes + 15) // 16 * 16


def test_pad_then_decode_rows():
    import torch
    t, o = _pair("cl100k_base")
    texts = fuzz_corpus(78, 200) + [""]
    dv, batch = _encode(t, texts)
    L = 48
    bos, eos = o.special_tokens["<|endofprompt|>"], o.special_tokens["<|endoftext|>"]
    n_tok = (batch.out_off[1:] - batch.out_off[:-1]).cpu().tolist()
    for side in ("right", "left"):
        rows, mask, lens = dv.pad_device(t, batch, L, pad_id=9906, bos_id=bos, eos_id=eos, padding_side=side, dtype=torch.int64)     # (the pad id would decode)
        out, off = dv.decode_rows_device(t, rows, lens, max_bytes=batch.n_bytes, padding_side=side, skip_special_tokens=True)
        o_h, raw = off.cpu().tolist(), out.cpu().numpy().tobytes()
        whole = [i for i, n in enumerate(n_tok) if n <= L - 2]
        assert len(whole) > 20 and len(whole) < len(texts)
        for i in whole:                                   # rows that were not truncated give their text back
            assert raw[o_h[i]:o_h[i + 1]] == texts[i].encode("utf-8"), (side, i)
        with_sp = dv.decode_rows_device(t, rows, lens, max_bytes=batch.n_bytes + 64 * len(texts), padding_side=side)[1]
        assert int(with_sp[-1]) == o_h[-1] + len(texts) * len(b"<|endofprompt|><|endoftext|>")


def test_transcode_on_one_stream():
    """cl100k ids -> bytes -> o200k ids: the decode's output IS the device encode's input; nothing crosses to the host in between"""
    import torch
    from splintr_amd import _ffi
    ta, _ = _pair("cl100k_base")
    tb, _ = _pair("o200k_base")
    texts = fuzz_corpus(79, 150) + ["", "Hello, world!"]
    texts.append("x" * ((5 - sum(len(x.encode("utf-8")) for x in texts)) % 16 + 16))       # the text ends 5 bytes into a 16-byte group
    dv, batch = _encode(ta, texts)
    out, off = dv.decode_device(ta, batch.ids, batch.out_off, max_bytes=batch.n_bytes)
    assert out.numel() == (batch.n_bytes + 15) // 16 * 16 and batch.n_bytes % 16 == 5
    out[batch.n_bytes:] = 0xA5                            # the decode leaves the tail of the last 16-byte group unwritten: the encoder needs it readable, no more
    ids_b = torch.empty(max(batch.n_bytes, 1), dtype=torch.int32, device=_dev())
    off_b = torch.empty(len(texts) + 1, dtype=torch.int64, device=_dev())
    rc = _ffi.lib().spl_encode_batch_device(tb.handle, out.data_ptr(), batch.n_bytes, off.data_ptr(), len(texts), 0, ids_b.data_ptr(),
                                            ids_b.numel(), off_b.data_ptr(), torch.cuda.current_stream(_dev()).cuda_stream)
    assert rc == 0, _ffi.last_error()
    o_h = off_b.cpu().tolist()
    got = ids_b[:o_h[-1]].cpu().tolist()
    assert [got[o_h[i]:o_h[i + 1]] for i in range(len(texts))] == tb.encode_batch(texts)


def test_same_bytes_as_the_host_path():
    import torch
    from splintr_amd import corpus
    from splintr_amd import device as dv
    t, o = _pair("o200k_base")
    enc = t.encode_batch(corpus.c3(300, seed=8))
    n = sum(map(len, enc))
    assert n > 80000
    want = t._decode_batch_bytes(enc)
    off = np.zeros(len(enc) + 1, dtype=np.int64)
    np.cumsum([len(e) for e in enc], out=off[1:])
    ids = torch.from_numpy(np.fromiter((x for e in enc for x in e), dtype=np.uint32, count=n).view(np.int32)).to(_dev())
    out, oo = dv.decode_device(t, ids, torch.from_numpy(off).to(_dev()), max_bytes=sum(map(len, want)))
    o_h, raw = oo.cpu().tolist(), out.cpu().numpy().tobytes()
    assert [raw[o_h[i]:o_h[i + 1]] for i in range(len(enc))] == want


def test_reserved_calls_reuse_their_scratch():
    from splintr_amd import Tokenizer
    from splintr_amd import device as dv
    t = Tokenizer.from_pretrained("cl100k_base")          # a handle of our own: its scratch starts empty
    _, o = _pair("cl100k_base")
    dv.decode_reserve(t, 5000)
    rng = random.Random(16)
    for n in (4000, 1200, 5000, 60000, 300):              # two within the reserve, its edge, one larger (not reserved for), a small one again
        ids = _mixed_ids(o, rng, n, p_unknown=0.05)
        off = _split(rng, n, 12)
        w_raw, w_off = _want_csr(o, ids, off, n)
        raw, oo = _call(t, ids, n, off, None, 12, 0, 0, len(w_raw))
        assert oo == w_off and raw == w_raw, n


def test_decode_tensor():
    import torch
    t, o = _pair("cl100k_base")
    ids = t.encode("你好世界")                              # 世 is split over two tokens
    rows = torch.tensor([ids, ids[:3] + [9906, 9906]], dtype=torch.int64, device=_dev())
    lens = torch.tensor([5, 3], dtype=torch.int32, device=_dev())
    assert t.decode_tensor(rows[:1]) == ["你好世界"]
    with pytest.raises(ValueError, match="invalid UTF-8"):
        t.decode_tensor(rows, lens)
    lossy = o.decode_bytes(ids[:3]).decode("utf-8", "replace")
    assert t.decode_tensor(rows, lens, errors="replace") == ["你好世界", lossy]
    assert t.decode_tensor(rows, errors="replace") == ["你好世界", lossy + "HelloHello"]
    left = torch.tensor([ids, [9906, 9906] + ids[:3]], dtype=torch.int32, device=_dev())
    assert t.decode_tensor(left, lens, padding_side="left", errors="replace") == ["你好世界", lossy]
    sp = o.special_tokens["<|endoftext|>"]
    r = torch.tensor([[sp, 9906, -100, sp]], dtype=torch.int64, device=_dev())
    assert t.decode_tensor(r) == ["<|endoftext|>Hello<|endoftext|>"] and t.decode_tensor(r, skip_special_tokens=True) == ["Hello"]
    # a guess that is too small (6 bytes per id): ids of the 300-byte key -- the call runs a second time with the exact size
    tl, ol = _pair("lengths")
    long_id = next(i for k, i in ol.encoder.items() if len(k) == 300)
    got = tl.decode_tensor(torch.full((3, 40), long_id, dtype=torch.int32, device=_dev()))
    assert got == [ol.decode_bytes([long_id] * 40).decode()] * 3 and len(got[0]) == 12000
