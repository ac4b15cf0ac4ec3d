"""GPU tests (-m gpu) of spl_token_spans_device (csrc/spl_k_spans.h): per id a byte span and a character span inside its document, and
the documents' offsets -- for a CSR or rows of ids in HBM.

Expected: tests/spans_ref.py over what the Python oracle decodes every id to.  Every output lies in an allocation longer than what the
call may write, filled with 0xA5: each check asserts that everything behind still holds it.  For every case the byte offsets are also
held against spl_decode_batch_device's d_out_off for the same input, and every token's byte span against the bytes that call wrote.
Shapes are the smallest at which each mechanism can go wrong: id counts around the 1 024-slot block, one document over three blocks,
5 000 empty documents; the mapping itself is tested exhaustively on the CPU (tests/test_spans_cpu.py)."""
import ctypes
import os
import random

import numpy as np
import pytest

import spans_ref as ref
from conftest import ROOT
from decode_ref import I64, PAD_LEFT, SKIP_SPECIAL
from fuzzgen import fuzz_corpus
from test_gpu_decode_device import _call as _decode_call, _dev, _holes_pair, _mixed_ids, _pair, _special_only, _split
from test_host_regex import SPARSE

pytestmark = pytest.mark.gpu

TAIL = 16                                   # span entries behind `slots`
POISON32 = np.int32(-0x5A5A5A5B)            # 0xA5A5A5A5
OFF_POISON = -0x5A5A5A5A5A5A5A5B
SPL_EINVAL = -1
PINNED = {"cl100k_base": [("世界", [0, 0, 1]), ("🧑‍🚀", [0, 0, 0, 1, 1, 2, 2, 2]), ("naïve ☃", [0, 2, 3, 5, 6]), ("𓀀", [0, 0, 0, 0])],
          "o200k_base": [("🧑‍🚀", [0, 0, 0, 1, 2, 2])]}
PINNED_LENS = {("cl100k_base", "世界"): (2, 1, 3), ("o200k_base", "🧑‍🚀"): (2, 1, 1, 3, 3, 1), ("cl100k_base", "naïve ☃"): (2, 2, 2, 3, 1),
               ("cl100k_base", "𓀀"): (1, 1, 1, 1)}


class _OracleTable:
    """what spans_ref needs of decode_ref.Table, over the Python oracle: one id value -> the bytes the decode emits for it"""

    def __init__(self, o):
        self.o, self.special_only, self.memo = o, _special_only(o), {}

    def span(self, v, flags):
        v = int(v)
        if not flags & I64:
            v &= 0xFFFFFFFF
        if not 0 <= v < (1 << 32) or (flags & SKIP_SPECIAL and v in self.special_only):
            return b""
        if v not in self.memo:
            self.memo[v] = self.o.decode_bytes([v])
        return self.memo[v]


_tabs = {}


def _tab(name, o):
    if name not in _tabs:
        _tabs[name] = _OracleTable(o)
    return _tabs[name]


# ------------------------------------------------------------------------------------------ one call into guarded buffers
def _call(t, ids, n_cap, off, lens, n_docs, flags, row_len, i64=False, null=()):
    """-> (byte_span | None, char_span | None, byte_off, char_off | None) as numpy; null: the outputs passed as NULL"""
    import torch
    from splintr_amd import _ffi
    dev = _dev()
    ids = np.ascontiguousarray(ids)
    if ids.dtype == np.uint32:
        ids = ids.view(np.int32)
    d_ids = torch.from_numpy(np.concatenate([ids.reshape(-1), np.zeros(4, ids.dtype)])).to(dev)           # (never a null pointer)
    d_off = None if off is None else torch.from_numpy(np.asarray(off).astype(np.int64)).to(dev)
    d_len = None if lens is None else torch.from_numpy(np.asarray(lens).astype(np.int32)).to(dev)
    slots = n_docs * row_len if row_len else n_cap
    W = 4 if i64 else 2
    span = lambda: torch.full(((slots + TAIL) * W,), int(POISON32), dtype=torch.int32, device=dev)
    offs = lambda: torch.full((n_docs + 2,), OFF_POISON, dtype=torch.int64, device=dev)
    bs, cs, bo, co = span(), span(), offs(), offs()
    p = lambda x, key: None if key in null else x.data_ptr()
    o = _ffi.SplDecodeOpts(flags, row_len)
    rc = _ffi.lib().spl_token_spans_device(t.handle, d_ids.data_ptr(), n_cap, None if d_off is None else d_off.data_ptr(),
                                           None if d_len is None else d_len.data_ptr(), n_docs, ctypes.byref(o), 1 if i64 else 0,
                                           p(bs, "bs"), p(cs, "cs"), bo.data_ptr(), p(co, "co"), torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, _ffi.last_error()
    out = []
    for x, key in ((bs, "bs"), (cs, "cs")):
        h = x.cpu().numpy()
        if key in null:
            assert (h == POISON32).all(), "a NULL output's stand-in was written"
            out.append(None)
            continue
        assert (h[slots * W:] == POISON32).all(), "written at or beyond `slots`"
        out.append(h[:slots * W].view(np.int64 if i64 else np.int32).reshape(slots, 2))
    for x, key in ((bo, "bo"), (co, "co")):
        h = x.cpu().numpy()
        if key in null:
            assert (h == OFF_POISON).all()
            out.append(None)
            continue
        assert h[-1] == OFF_POISON, "written behind the offsets"
        out.append(h[:-1].astype(np.uint64))
    return tuple(out)


def _same(got, want, tag):
    for g, w, what in zip(got, want, ("byte_span", "char_span", "byte_off", "char_off")):
        if g is not None:
            assert g.dtype == w.dtype and np.array_equal(g, w), (tag, what, np.argwhere(g != w)[:4].tolist())


def _check_csr(name, ids, off, tag, *, n_cap=None, flags=0, i64=False, null=(), pair=None):
    t, o = pair or _pair(name)[:2]
    ids = np.asarray(ids)
    off = np.asarray(off, dtype=np.uint64)
    n_cap = len(ids) if n_cap is None else n_cap
    n_docs = len(off) - 1
    got = _call(t, ids, n_cap, off, None, n_docs, flags, 0, i64, null)
    tab = _tab(name, o)
    _same(got, ref.spans_csr(tab, ids, off, n_cap, flags, i64), tag)
    # the decode of the same input: its offsets are byte_off, and every token's byte span indexes its bytes
    need = int(got[2][-1])
    raw, d_off = _decode_call(t, ids, n_cap, off, None, n_docs, flags, 0, need)
    assert d_off == got[2].tolist(), (tag, "byte_off != the decode's d_out_off")
    if got[0] is not None:
        c = [min(int(x), n_cap) for x in off]
        for d in range(n_docs):
            for i in range(c[d], c[d + 1]):
                s, e = got[0][i]
                assert raw[d_off[d] + s:d_off[d] + e] == tab.span(ids[i], flags), (tag, d, i)
    return got


# ------------------------------------------------------------------------------------------ block edges, documents, outputs
@pytest.mark.parametrize("name", ["cl100k_base", "deepseek_v3"])
def test_block_edges(name):
    t, o = _pair(name)
    rng = random.Random(21)
    for n in (0, 1, 1023, 1024, 1025, 2049):
        ids = _mixed_ids(o, rng, n)
        _check_csr(name, ids, [0, n], (name, n, "one document"), i64=bool(n & 1))
        _check_csr(name, ids, _split(rng, n, 7), (name, n, "seven documents"), flags=SKIP_SPECIAL)
        _check_csr(name, ids.astype(np.int64), _split(rng, n, 3), (name, n, "int64 ids"), flags=I64, i64=not n & 1)


def test_documents():
    name = "cl100k_base"
    t, o = _pair(name)
    rng = random.Random(22)
    z = np.zeros(0, dtype=np.uint32)
    got = _check_csr(name, z, [0], "n_docs = 0")
    assert got[2].tolist() == [0] and got[3].tolist() == [0]
    _check_csr(name, z, [0, 0, 0, 0], "three empty documents and no id")
    ids = _mixed_ids(o, rng, 3300, p_unknown=0.1)
    short = sorted(rng.randrange(100) for _ in range(6))
    _check_csr(name, ids, [0] + short + [100, 3100] + [3100 + 40 * k for k in range(1, 6)], "one document of 3 000 ids among short ones")
    for tag, off in (("5 000 empty first", [0] * 5000 + [1024, 2500]), ("5 000 empty at a block boundary", [0, 1024] + [1024] * 5000 + [2500]),
                     ("5 000 empty last", [0, 1000] + [2500] * 5000)):
        _check_csr(name, ids[:2500], off, tag)
    # the cap far above the count (slots of no document: (0, 0)) and the clamp below it
    off = _split(rng, 2048, 40)
    got = _check_csr(name, np.concatenate([ids[:2048], np.full(1000, 9906, np.uint32)]), off, "cap above the count")
    assert not got[0][2048:].any() and not got[1][2048:].any()
    for n_cap in (2047, 1024, 1):
        _check_csr(name, ids[:2048], off, ("clamp", n_cap), n_cap=n_cap)


def test_each_optional_output_null_and_both_widths():
    name = "cl100k_base"
    t, o = _pair(name)
    rng = random.Random(23)
    ids = _mixed_ids(o, rng, 1500)
    off = _split(rng, 1500, 9)
    for null in (("bs",), ("cs",), ("co",), ("bs", "cs", "co")):
        for i64 in (False, True):
            _check_csr(name, ids, off, (null, i64), null=null, i64=i64)


@pytest.mark.parametrize("shape", [(37, 65), (65, 37)])
def test_rows(shape):
    t, o = _pair("far")
    tab = _tab("far", o)
    n, row_len = shape
    rng = random.Random(row_len)
    rows = _mixed_ids(o, rng, n * row_len, p_unknown=0.1).astype(np.int64).reshape(n, row_len)      # padding slots hold ids that would decode
    rows.flat[::97] = 2 ** 31 - 1                                                                   # the far special
    lens = np.array([rng.randrange(-2, row_len + 3) for _ in range(n)], dtype=np.int32)
    lens[0], lens[n - 1], lens[n // 2] = 0, row_len, row_len + 100
    odd = rows.copy()
    odd.flat[::13] = [(-1, -100, 2 ** 32, 2 ** 32 + 17)[k & 3] for k in range(len(odd.flat[::13]))]
    r32 = rows.astype(np.uint32).view(np.int32)
    for r, ln, flags in ((rows, None, I64), (rows, lens, I64), (rows, lens, I64 | PAD_LEFT), (odd, lens, I64 | PAD_LEFT | SKIP_SPECIAL),
                         (r32, lens, 0), (r32, lens, PAD_LEFT)):
        got = _call(t, r, 0, None, ln, n, flags, row_len, i64=bool(flags & SKIP_SPECIAL))
        _same(got, ref.spans_rows(tab, r, ln, flags, bool(flags & SKIP_SPECIAL)), (shape, flags))
        need = int(got[2][-1])
        raw, d_off = _decode_call(t, r, 0, None, ln, n, flags, row_len, need)
        assert d_off == got[2].tolist(), (shape, flags)
        for i in range(0, n * row_len, 7):                 # (a sample: a padding slot's span is empty)
            s, e = got[0][i]
            d = i // row_len
            k = row_len if ln is None else max(0, min(int(ln[d]), row_len))
            c = i % row_len
            valid = c >= row_len - k if flags & PAD_LEFT else c < k
            assert raw[d_off[d] + s:d_off[d] + e] == (tab.span(r.reshape(-1)[i], flags) if valid else b""), (shape, flags, i)


def test_skip_special_and_long_keys():
    rng = random.Random(24)
    # the far specials of a shipped vocabulary, skipped and not (the side table's character counts: a 255-byte literal)
    ids = np.array([9906, 100257, 11, 100300, 100301, 1917, 5_000_000, 2 ** 31 - 1, 0, 100262, 4_999_999] * 100, dtype=np.uint32)
    for flags in (0, SKIP_SPECIAL):
        _check_csr("far", ids, _split(rng, len(ids), 5), ("far specials", flags), flags=flags)
    # specials in a hole of the dense range, on a vocabulary id, far away -- over the `lengths` vocabulary
    t, o, hole, both = _holes_pair()
    known = sorted(o.encoder.values())
    unit = [hole[0], both, known[3], hole[2], 2 ** 31 - 1, hole[1], both, 2 ** 31 - 2, known[40]]
    for flags in (0, SKIP_SPECIAL):
        _check_csr("holes", np.array(unit * 130, dtype=np.uint32), _split(rng, len(unit) * 130, 11), ("holes", flags), flags=flags, pair=(t, o))
    # 300-byte keys: one block is 307 200 bytes
    tl, ol = _pair("lengths")
    long_id = next(i for k, i in ol.encoder.items() if len(k) == 300)
    got = _check_csr("lengths", np.full(1100, long_id, dtype=np.uint32), [0, 1, 1024, 1100], "300-byte key")
    assert got[2].tolist() == [0, 300, 307200, 330000] and got[0][1023].tolist() == [1022 * 300, 1023 * 300]
    kn = sorted(ol.encoder.values())
    ids = np.array([rng.choice(kn) for _ in range(2500)] + [2 ** 21 - 2, 2 ** 21 - 1, 2 ** 21], dtype=np.uint32)
    _check_csr("lengths", ids, _split(rng, len(ids), 9), "sparse ids up to 2^21 - 2")


def test_python_wrappers_with_every_argument():
    """device.spans_device / spans_rows_device called directly: chars=False, int64 spans, lengths with both padding sides, skipped specials"""
    import torch
    from splintr_amd import device as dv
    t, o = _pair("far")
    tab = _tab("far", o)
    dev = _dev()
    rng = random.Random(25)
    ids = _mixed_ids(o, rng, 1300, p_unknown=0.1)
    ids[::50] = 100300
    off = _split(rng, 1300, 6)
    d_ids, d_off = torch.from_numpy(ids.view(np.int32)).to(dev), torch.from_numpy(off.astype(np.int64)).to(dev)
    for skip in (False, True):
        flags = SKIP_SPECIAL if skip else 0
        want = ref.spans_csr(tab, ids, off, 1300, flags, True)
        bs, cs, bo, co = dv.spans_device(t, d_ids, d_off, chars=False, dtype=torch.int64, skip_special_tokens=skip)
        assert cs is None and co is None and bs.dtype == torch.int64
        assert np.array_equal(bs.cpu().numpy(), want[0]) and bo.cpu().tolist() == want[2].tolist(), skip
        out, d_out_off = dv.decode_device(t, d_ids, d_off, max_bytes=int(want[2][-1]), skip_special_tokens=skip)
        assert torch.equal(d_out_off, bo)
        got = dv.spans_device(t, d_ids.long(), d_off, skip_special_tokens=skip)
        w32 = ref.spans_csr(tab, ids, off, 1300, flags)
        assert all(np.array_equal(g.cpu().numpy().astype(w.dtype), w) for g, w in zip(got, w32)) and got[1].dtype == torch.int32
    rows = _mixed_ids(o, rng, 9 * 41, p_unknown=0.1).astype(np.int64).reshape(9, 41)
    lens = np.array([0, 41, 50, -1, 7, 40, 1, 20, 33], dtype=np.int32)
    d_rows, d_lens = torch.from_numpy(rows).to(dev), torch.from_numpy(lens).to(dev)
    for side in ("right", "left"):
        for skip in (False, True):
            flags = I64 | (PAD_LEFT if side == "left" else 0) | (SKIP_SPECIAL if skip else 0)
            got = dv.spans_rows_device(t, d_rows, d_lens, padding_side=side, dtype=torch.int64, skip_special_tokens=skip)
            want = ref.spans_rows(tab, rows, lens, flags, True)
            assert all(np.array_equal(g.cpu().numpy().astype(w.dtype), w) for g, w in zip(got, want)), (side, skip)
            bs, cs, bo, co = dv.spans_rows_device(t, d_rows, d_lens, padding_side=side, chars=False, skip_special_tokens=skip)
            assert cs is None and co is None and np.array_equal(bs.cpu().numpy(), ref.spans_rows(tab, rows, lens, flags)[0])
    got = dv.spans_rows_device(t, d_rows)
    assert all(np.array_equal(g.cpu().numpy().astype(w.dtype), w) for g, w in zip(got, ref.spans_rows(tab, rows, None, I64)))
    e = dv.spans_rows_device(t, torch.zeros(3, 0, dtype=torch.int64, device=dev))
    assert e[0].shape == (0, 2) and e[2].tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------ end to end, from texts
def _texts(name):
    return [x for x, _ in PINNED["cl100k_base"]] + ["", "Hello, world!", "don't — “quoted” it’s", "こんにちは 世界 🦀"] + fuzz_corpus(31, 150) + [""]


@pytest.mark.parametrize("name", ["cl100k_base", "o200k_base", "deepseek_v3"])
def test_encode_batch_with_offsets(name, coracle):
    t, o = _pair(name)
    texts = _texts(name)
    want = coracle(name).encode_batch(texts)
    ids, bspans = t.encode_batch_with_offsets(texts, unit="byte")
    ids2, cspans = t.encode_batch_with_offsets(texts)
    assert ids == want and ids2 == want
    tab = _tab(name, o)
    for d, text in enumerate(texts):
        raw = text.encode("utf-8")
        assert len(bspans[d]) == len(cspans[d]) == len(ids[d])
        prev = 0
        for k, tid in enumerate(ids[d]):
            s, e = bspans[d][k]
            assert s == prev and raw[s:e] == tab.span(tid, 0), (name, d, k)               # the byte spans tile the text
            prev = e
            cs, ce = cspans[d][k]
            piece = text[cs:ce].encode("utf-8")                                          # str indices: the characters the token touches, no more
            assert raw[s:e] in piece and len(text[:cs].encode("utf-8")) <= s and len(text[:ce].encode("utf-8")) >= e, (name, d, k)
            assert ce - cs < 2 or (len(text[:cs + 1].encode("utf-8")) > s and len(text[:ce - 1].encode("utf-8")) < e), (name, d, k)
        assert prev == len(raw)
    if name != "deepseek_v3":
        ids3, sp3 = t.encode_batch_with_offsets(["a<|endoftext|>b"], with_special=True)
        assert ids3 == coracle(name).encode_batch(["a<|endoftext|>b"], with_special=True) and sp3 == [[(0, 1), (1, 14), (14, 15)]]
    assert t.encode_batch_with_offsets([]) == ([], [])


@pytest.mark.parametrize("name", ["cl100k_base", "o200k_base"])
def test_decode_with_offsets_matches_the_pinned_tiktoken_starts(name):
    t, o = _pair(name)
    tab = _tab(name, o)
    for text, starts in PINNED[name]:
        ids = t.encode(text)
        lens = PINNED_LENS.get((name, text))
        if lens:
            assert tuple(len(tab.span(i, 0)) for i in ids) == lens, (name, text)
        assert t.decode_with_offsets(ids) == (text, starts), (name, text)
        assert t.encode_batch_with_offsets([text])[1][0] and [s for s, _ in t.encode_batch_with_offsets([text])[1][0]] == starts
    assert t.decode_with_offsets([]) == ("", [])
    with pytest.raises(ValueError, match="invalid UTF-8"):
        t.decode_with_offsets(t.encode("🧑‍🚀")[:1])          # (both vocabularies split the first character three ways)


def test_a_pattern_that_leaves_gaps_is_detected():
    from splintr_amd import Tokenizer
    with open(os.path.join(ROOT, "splintr_amd", "data", "cl100k_base.splv"), "rb") as f:
        t = Tokenizer.from_bytes(f.read(), SPARSE)
    ids, spans = t.encode_batch_with_offsets(["nogaps", "", "abc"], unit="byte")
    assert [s[-1][1] if s else 0 for s in spans] == [6, 0, 3]
    with pytest.raises(ValueError, match="document 2 is 10 bytes of UTF-8 but its ids decode to 5"):
        t.encode_batch_with_offsets(["tiles", "", "  ab, 12x!", "???"])


# ------------------------------------------------------------------------------------------ refusals: nothing is written
def test_refusals_write_nothing():
    import torch
    from splintr_amd import _ffi
    t, o = _pair("cl100k_base")
    dev = _dev()
    L = _ffi.lib()
    ids = torch.full((64,), 9906, dtype=torch.int32, device=dev)
    off = torch.tensor([0, 10, 64], dtype=torch.int64, device=dev)
    lens = torch.tensor([3, 4], dtype=torch.int32, device=dev)
    outs = [torch.full((64 * 4 + 8,), int(POISON32), dtype=torch.int32, device=dev) for _ in range(2)] + \
           [torch.full((4,), OFF_POISON, dtype=torch.int64, device=dev) for _ in range(2)]
    O = _ffi.SplDecodeOpts

    def call(o=None, sf=0, i=ids.data_ptr(), f=off.data_ptr(), ln=None, bs=outs[0].data_ptr(), cs=outs[1].data_ptr(), bo=outs[2].data_ptr(),
             n=2, cap=64):
        o = O(0, 0) if o is None else o
        return L.spl_token_spans_device(t.handle, i, cap, f, ln, n, ctypes.byref(o), sf, bs, cs, bo, outs[3].data_ptr(),
                                        torch.cuda.current_stream(dev).cuda_stream)

    short = O(0, 0)
    short.struct_size = 8
    for kw, word in ((dict(sf=2), "span_flags"), (dict(bo=None), "d_byte_off is null"), (dict(bs=outs[0].data_ptr() + 8), "d_byte_span"),
                     (dict(cs=outs[1].data_ptr() + 4), "d_char_span"), (dict(o=O(8, 0)), "unknown flag bit"), (dict(o=short), "struct_size"),
                     (dict(o=O(PAD_LEFT, 0)), "PAD_LEFT"), (dict(ln=lens.data_ptr()), "d_len"), (dict(f=None), "d_ids_off is null"),
                     (dict(o=O(0, 32)), "d_ids_off"), (dict(i=ids.data_ptr() + 4), "16-byte"), (dict(i=None), "d_ids is null"),
                     (dict(n=1 << 31), "n_docs"), (dict(cap=1 << 41), "2^41")):
        rc = call(**kw)
        assert rc == SPL_EINVAL and word in _ffi.last_error(), (rc, word, _ffi.last_error())
    torch.cuda.synchronize(dev)
    assert all(bool((x == int(POISON32)).all()) for x in outs[:2]) and all(bool((x == OFF_POISON).all()) for x in outs[2:])
    assert call() == 0                                    # (the same buffers are fine for a call that is not refused)
    torch.cuda.synchronize(dev)
    assert outs[2].tolist()[:3] == [0, 50, 320] and outs[2].tolist()[3] == OFF_POISON
