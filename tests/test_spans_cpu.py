"""spl_token_spans_device without a GPU: the C ABI's symbol and refusals, the Python surface's ValueErrors, tests/spans_ref.py against
tiktoken's decode_with_offsets convention written out by hand, and the mapping code the kernels run (splintr_amd/csrc/spl_k_spans.h,
evaluated block by block and lane by lane by tests/hostsim/spans_sim.cpp) against spans_ref -- on decode_ref's synthetic table (token
lengths 0 .. 300, arbitrary bytes) and on a table of UTF-8 pieces that split characters.  Every case also holds byte_off against the
decode simulation's out_off for the same input.  Two mutants of the driver each fail named cases."""
import ctypes
import os
import re

import numpy as np
import pytest

import decode_ref
import spans_ref as ref
from decode_ref import I64, PAD_LEFT, SKIP_SPECIAL
from conftest import ROOT

SPL_EINVAL = -1
INT32_MAX = (1 << 31) - 1


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as entry
    entry.build()
    from splintr_amd import _ffi
    return _ffi


@pytest.fixture(scope="module")
def sim():
    import spans_sim
    spans_sim.lib()
    return spans_sim


@pytest.fixture(scope="module")
def dsim():
    import decode_sim
    decode_sim.lib()
    return decode_sim


# ------------------------------------------------------------------------------------------ the tables
U_MAX_ID = 31
U_FAR = 100300
SEJIE, ZWJ = "世界".encode(), "🧑‍🚀".encode()
# ids 3 4 5: 世界 as (2, 1, 3); 6 .. 12: the pieces of 🧑 ZWJ 🚀 (2 1 1 | 2 1 | 2 1 1, ids 6 7 8 9 10 6 11 12); 20 and U_FAR special-only
U_TOKENS = {0: b"", 1: b"a", 2: "é".encode(), 3: SEJIE[:2], 4: SEJIE[2:3], 5: SEJIE[3:], 6: ZWJ[:2], 7: ZWJ[2:3], 8: ZWJ[3:4], 9: ZWJ[4:6],
            10: ZWJ[6:7], 11: ZWJ[9:10], 12: ZWJ[10:11], 13: b" hello", 14: b"x" * 300, 15: "ï".encode()[1:] + b"b", 20: b"<|s|>",
            U_FAR: "<|far é|>".encode()}
U_KNOWN = sorted(U_TOKENS)
U_UNKNOWN = [16, 19, 21, 31, 32, 77, U_FAR - 1, U_FAR + 1, 0xFFFFFFFF]


@pytest.fixture(scope="module")
def tabs(sim):
    """[(Table, SpanTable)]: decode_ref's synthetic table, and the UTF-8 pieces"""
    syn = decode_ref.synthetic_table()
    utf = decode_ref.Table(U_TOKENS, special_only={20, U_FAR})
    return [(syn, sim.SpanTable(syn, decode_ref.SYN_MAX_ID)), (utf, sim.SpanTable(utf, U_MAX_ID))]


def _ids(rng, which, n, p_unknown=0.25):
    if which == 0:
        return decode_ref.random_ids(rng, n, p_unknown)
    out = np.empty(n, dtype=np.uint32)
    for i in range(n):
        pool = U_UNKNOWN if rng.random() < p_unknown else U_KNOWN
        out[i] = pool[int(rng.integers(len(pool)))]
    return out


def _split(rng, n, n_docs):
    cuts = np.sort(rng.integers(0, n + 1, size=max(n_docs - 1, 0)))
    return np.concatenate([[0], cuts, [n]]).astype(np.uint64) if n_docs else np.zeros(1, dtype=np.uint64)


def _same(got, want, what):
    bs, cs, bo, co = got[:4]
    assert bo.tolist() == want[2].tolist(), (what, "byte_off")
    if co is not None:
        assert co.tolist() == want[3].tolist(), (what, "char_off")
    if bs is not None:
        assert bs.dtype == want[0].dtype and np.array_equal(bs, want[0]), (what, "byte_span", np.argwhere(bs != want[0])[:4].tolist())
    if cs is not None:
        assert cs.dtype == want[1].dtype and np.array_equal(cs, want[1]), (what, "char_span", np.argwhere(cs != want[1])[:4].tolist())


def _check_csr(sim, dsim, pair, ids, off, what, *, flags=0, n_cap=None, poison_tail=0, lanes=None, i64=False, want=(1, 1, 1), mutant=0):
    """spans_sim == spans_ref for a CSR, and byte_off == decode_sim's out_off; poison_tail: ids behind the count that would decode"""
    tab, st = pair
    ids = np.asarray(ids)
    buf = np.concatenate([ids, np.full(poison_tail, 4, dtype=ids.dtype)]) if poison_tail else ids
    cap = len(buf) if n_cap is None else n_cap
    got = sim.spans(st, buf, off, n_cap=cap, flags=flags, i64=i64, lanes=lanes, want=want, mutant=mutant)
    _same(got, ref.spans_csr(tab, buf, off, cap, flags, i64), what)
    _, d_off, _ = dsim.decode(st, buf, off, n_cap=cap, flags=flags, capacity=0, lanes=lanes)
    assert got[2].tolist() == d_off.tolist(), (what, "byte_off != the decode's out_off")
    return got[4]


def _check_rows(sim, dsim, pair, rows, lens, what, *, flags=0, lanes=None, i64=False):
    tab, st = pair
    got = sim.spans(st, rows, None, lens, row_len=rows.shape[1], flags=flags, i64=i64, lanes=lanes)
    _same(got, ref.spans_rows(tab, rows, lens, flags, i64), what)
    _, d_off, _ = dsim.decode(st, rows, None, lens, row_len=rows.shape[1], flags=flags, capacity=0, lanes=lanes)
    assert got[2].tolist() == d_off.tolist(), (what, "byte_off != the decode's out_off")
    return got[4]


# ------------------------------------------------------------------------------------------ 1. the C ABI
def test_symbol_flag_and_argument_types(ffi):
    L = ffi.lib()
    assert "spl_token_spans_device" in ffi.SYMBOLS and hasattr(L, "spl_token_spans_device")
    hdr = open(os.path.join(ROOT, "include", "splintr_hip.h")).read()
    assert re.search(r"#define SPL_SPANS_I64\s+1u\b", hdr) and ffi.SPL_SPANS_I64 == 1
    decl = re.search(r"int spl_token_spans_device\((.*?)\);", hdr, re.S).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert args == ["spl_tokenizer* t", "const void* d_ids", "uint64_t n_ids_cap", "const uint64_t* d_ids_off", "const int32_t* d_len",
                    "uint64_t n_docs", "const spl_decode_opts* o", "uint32_t span_flags", "void* d_byte_span", "void* d_char_span",
                    "uint64_t* d_byte_off", "uint64_t* d_char_off", "void* hip_stream"]
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    assert L.spl_token_spans_device.argtypes == [vp, vp, u64, vp, vp, u64, ctypes.POINTER(ffi.SplDecodeOpts), ctypes.c_uint32] + [vp] * 5
    for word in ("decode_with_offsets", "d_byte_off[d + 1] - d_byte_off[d]", "(0, 0)", "INT32_MAX"):
        assert word in hdr, word                       # the convention, the caller's check, the slots of no document, the saturation


def test_refusals_name_their_cause(ffi):
    """Every refusal comes before the handle or the device is touched: a dummy handle (never read) is enough, and none of the addresses
    below is ever dereferenced.  The input's refusals are the decode's, word for word."""
    L = ffi.lib()
    handle = ctypes.create_string_buffer(64)
    h = ctypes.addressof(handle)
    A = 0x10000
    O = ffi.SplDecodeOpts
    NIL = "nil"

    def call(t=h, ids=A, cap=100, off=NIL, ln=None, n=3, o=None, sf=0, bs=A, cs=A, bo=A, co=A):
        o = O(0, 0) if o is None else o
        if off is NIL:
            off = None if (o is not False and o.row_len) else A
        return L.spl_token_spans_device(t, ids, cap, off, ln, n, ctypes.byref(o) if o is not False else None, sf, bs, cs, bo, co, None)

    def refused(rc, *words):
        msg = L.spl_last_error().decode()
        assert rc == SPL_EINVAL, (rc, msg)
        for w in ("spl_token_spans_device",) + words:
            assert w in msg, (w, msg)

    refused(call(t=None), "null handle")
    refused(call(o=False), "options")
    refused(call(ids=None), "d_ids is null")
    refused(call(ids=None, o=O(0, 8)), "d_ids is null")
    short = O(0, 0)
    for size in (0, 8, 4097):
        short.struct_size = size
        refused(call(o=short), "struct_size")
    refused(call(o=O(8, 0)), "unknown flag bit 0x8")
    refused(call(o=O(PAD_LEFT, 0)), "SPL_DECODE_PAD_LEFT", "CSR mode")
    refused(call(ln=A), "d_len", "CSR mode")
    refused(call(off=None), "d_ids_off is null", "CSR mode")
    refused(call(o=O(0, 8), off=A), "d_ids_off", "rows mode")
    refused(call(ids=A + 4), "d_ids", "16-byte")
    refused(call(ids=A + 16, o=O(I64, 0)), "d_ids", "32-byte")
    refused(call(n=1 << 31), "n_docs >= 2^31")
    refused(call(cap=1 << 41), "n_ids_cap", "2^41")
    refused(call(n=1 << 30, o=O(0, 1 << 11)), "n_docs * row_len", "2^41")
    # its own
    refused(call(sf=2), "unknown span_flags bit 0x2")
    refused(call(sf=0x80000001), "unknown span_flags bit 0x80000000")
    refused(call(bo=None), "d_byte_off is null")
    refused(call(bs=A + 8), "d_byte_span", "16-byte")
    refused(call(cs=A + 8, sf=1), "d_char_span", "16-byte")


def test_python_surface_validates_before_anything_goes_to_the_device():
    torch = pytest.importorskip("torch")
    from splintr_amd import device as dv
    ids = torch.zeros(8, dtype=torch.int32)
    off = torch.tensor([0, 8], dtype=torch.int64)
    with pytest.raises(ValueError, match="dtype must be torch.int32 or torch.int64"):
        dv.spans_device(None, ids, off, dtype=torch.int16)
    with pytest.raises(ValueError, match="int32 or int64"):
        dv.spans_device(None, ids.to(torch.int16), off)
    with pytest.raises(ValueError, match="offsets"):
        dv.spans_device(None, ids, off.to(torch.int32))
    with pytest.raises(ValueError, match="on a GPU"):
        dv.spans_device(None, ids, off)
    with pytest.raises(ValueError, match="rank 2"):
        dv.spans_rows_device(None, ids)
    with pytest.raises(ValueError, match="padding_side"):
        dv.spans_rows_device(None, ids.reshape(2, 4), padding_side="middle")
    with pytest.raises(ValueError, match="on a GPU"):
        dv.spans_rows_device(None, ids.reshape(2, 4), torch.tensor([1, 2], dtype=torch.int32))
    from splintr_amd import Tokenizer
    with pytest.raises(ValueError, match="unit"):
        Tokenizer.encode_batch_with_offsets(None, ["a"], unit="word")


# ------------------------------------------------------------------------------------------ 2. the convention, by hand
def _pieces(text, lens):
    b = text.encode()
    assert sum(lens) == len(b)
    cuts = np.concatenate([[0], np.cumsum(lens)])
    return [b[cuts[i]:cuts[i + 1]] for i in range(len(lens))]


PINNED = [("世界", (2, 1, 3), [0, 0, 1]),                                         # cl100k
          ("🧑‍🚀", (2, 1, 1, 2, 1, 2, 1, 1), [0, 0, 0, 1, 1, 2, 2, 2]),       # cl100k: 8 tokens
          ("🧑‍🚀", (2, 1, 1, 3, 3, 1), [0, 0, 0, 1, 2, 2]),                   # o200k
          ("naïve ☃", (2, 2, 2, 3, 1), [0, 2, 3, 5, 6]),                          # cl100k
          ("𓀀", (1, 1, 1, 1), [0, 0, 0, 0])]                                     # cl100k


@pytest.mark.parametrize("text,lens,starts", PINNED)
def test_ref_pins_tiktokens_character_starts(sim, text, lens, starts):
    """decode_with_offsets: a token that begins inside a character starts at that character -- the reference, and the mapping with it"""
    pieces = _pieces(text, lens)
    assert ref.char_starts(pieces) == starts
    tab = decode_ref.Table(dict(enumerate(pieces)))
    ids = np.arange(len(pieces), dtype=np.uint32)
    bs, cs, bo, co = ref.spans_csr(tab, ids, [0, len(ids)], len(ids))
    _same(sim.spans(sim.SpanTable(tab, len(pieces) + 2), ids, np.array([0, len(ids)], dtype=np.uint64), lanes=1), (bs, cs, bo, co), text)
    assert cs[:, 0].tolist() == starts
    assert bs[:, 0].tolist() == np.concatenate([[0], np.cumsum(lens)[:-1]]).tolist() and bs[:, 1].tolist() == np.cumsum(lens).tolist()
    assert bo.tolist() == [0, len(text.encode())] and co.tolist() == [0, len(text)]
    for i, p in enumerate(pieces):                   # the character span covers the token: str indices
        s, e = cs[i]
        assert p in text[s:e].encode() and (e - s < 2 or (p not in text[s + 1:e].encode() and p not in text[s:e - 1].encode()))
        assert text.encode()[bs[i, 0]:bs[i, 1]] == p


@pytest.mark.parametrize("text,lens,starts", PINNED)
def test_mapping_pins_tiktokens_character_starts(sim, dsim, text, lens, starts):
    pieces = _pieces(text, lens)
    tab = decode_ref.Table(dict(enumerate(pieces)))
    pair = (tab, sim.SpanTable(tab, len(pieces) + 2))
    ids = np.arange(len(pieces), dtype=np.uint32)
    for lanes in (1, 2, 256):
        got = sim.spans(pair[1], ids, np.array([0, len(ids)], dtype=np.uint64), lanes=lanes)
        assert got[1][:, 0].tolist() == starts, lanes
        _check_csr(sim, dsim, pair, ids, np.array([0, len(ids)], dtype=np.uint64), (text, lanes), lanes=lanes)


def test_ref_by_hand(sim, tabs):
    """the reference against spans written out by hand; the mapping is held against the same hand-written spans"""
    tab = decode_ref.Table(U_TOKENS, special_only={20, U_FAR})
    hand = np.array([4, 3, 77, 4, 5, 0, 20, 13, 1], dtype=np.uint32)
    got = sim.spans(tabs[1][1], hand, np.array([0, 0, 5, 6, 9], dtype=np.uint64), lanes=1)
    assert got[0].tolist() == [[0, 1], [1, 3], [3, 3], [3, 4], [4, 7], [0, 0], [0, 5], [5, 11], [11, 12]]
    assert got[1].tolist() == [[0, 0], [0, 1], [1, 1], [0, 1], [1, 2], [0, 0], [0, 5], [5, 11], [11, 12]]
    assert got[2].tolist() == [0, 0, 7, 7, 19] and got[3].tolist() == [0, 0, 2, 2, 14]
    ids = np.array([4, 3, 77, 4, 5, 0, 20, 13, 1], dtype=np.uint32)       # 4: a lone continuation byte; 77 unknown; 0 empty; 20 special
    bs, cs, bo, co = ref.spans_csr(tab, ids, [0, 0, 5, 6, 9], 9)
    #            doc 1: 96 | e4 b8 | - | 96 | e7 95 8c          doc 2: ""     doc 3: <|s|> " hello" a
    assert bs.tolist() == [[0, 1], [1, 3], [3, 3], [3, 4], [4, 7], [0, 0], [0, 5], [5, 11], [11, 12]]
    assert cs.tolist() == [[0, 0], [0, 1], [1, 1], [0, 1], [1, 2], [0, 0], [0, 5], [5, 11], [11, 12]]      # slot 0: cs == 0, the start stays 0
    assert bo.tolist() == [0, 0, 7, 7, 19] and co.tolist() == [0, 0, 2, 2, 14]
    bs, cs, bo, co = ref.spans_csr(tab, ids, [0, 0, 5, 6, 9], 9, SKIP_SPECIAL)
    assert bs[6:].tolist() == [[0, 0], [0, 6], [6, 7]] and bo.tolist() == [0, 0, 7, 7, 14]
    # clamped: the CSR claims 9 ids, the caller vouches for 7 -- slots at or beyond the clamped end do not exist
    bs, cs, bo, co = ref.spans_csr(tab, ids, [0, 0, 5, 6, 9], 7)
    assert len(bs) == 7 and bs[6].tolist() == [0, 5] and bo.tolist() == [0, 0, 7, 7, 12]
    # rows: padding slots are zero-length slots of their row
    rows = np.array([[1, 13, 2, 1], [2, 2, 2, 2]], dtype=np.uint32)
    bs, cs, bo, co = ref.spans_rows(tab, rows, [2, 9])
    assert bs.tolist() == [[0, 1], [1, 7], [7, 7], [7, 7], [0, 2], [2, 4], [4, 6], [6, 8]] and cs[4:].tolist() == [[0, 1], [1, 2], [2, 3], [3, 4]]
    bs, cs, bo, co = ref.spans_rows(tab, rows, [2, -1], PAD_LEFT)
    assert bs.tolist() == [[0, 0], [0, 0], [0, 2], [2, 3], [0, 0], [0, 0], [0, 0], [0, 0]] and bo.tolist() == [0, 3, 3] and co.tolist() == [0, 2, 2]


# ------------------------------------------------------------------------------------------ 3. the mapping against the reference
def test_mapping_exhaustive_small_blocks(sim, dsim, tabs):
    """Every id count 0 .. 40 with workgroups of 1, 2 and 3 lanes (blocks of 4, 8 and 12 slots): every block edge, the end at a multiple
    of the block, documents that run through several blocks (the carry-in), both tables, both span widths."""
    rng = np.random.default_rng(5111)
    cases, carries, reductions = 0, 0, 0
    for which, pair in enumerate(tabs):
        for lanes in (1, 2, 3):
            for n in range(41):
                for rep in range(3):
                    ids = _ids(rng, which, n, (0.25, 0.6, 0.0)[rep])
                    off = _split(rng, n, int(rng.integers(0, 7)))
                    key = (which, lanes, n, rep, ids.tolist(), off.tolist())
                    for flags in (0, SKIP_SPECIAL):
                        st = _check_csr(sim, dsim, pair, ids, off, key + (flags,), flags=flags, lanes=lanes, i64=bool(rep & 1))
                        carries += st["carries"]
                        reductions += st["carry_reductions"]
                        cases += 1
                    _check_csr(sim, dsim, pair, ids, off, key + ("tail",), lanes=lanes, poison_tail=int(rng.integers(1, 30)))
                    if n:
                        _check_csr(sim, dsim, pair, ids, off, key + ("clamp",), lanes=lanes, n_cap=int(rng.integers(0, n)))
                    v = ids.astype(np.int64)
                    if n:
                        v[int(rng.integers(n))] = (-1, -100, 1 << 32, (1 << 32) + 4)[rep + (n & 1)]
                    _check_csr(sim, dsim, pair, v, off, key + ("i64",), flags=I64, lanes=lanes)
    assert cases > 1400 and carries > 1000 and reductions > 500


def test_mapping_null_outputs(sim, dsim, tabs):
    rng = np.random.default_rng(5112)
    ids = _ids(rng, 1, 37)
    off = _split(rng, 37, 5)
    for want in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0)):
        for i64 in (False, True):
            _check_csr(sim, dsim, tabs[1], ids, off, (want, i64), lanes=2, want=want, i64=i64)


def _carry_case():
    """blocks of 4 slots; document 1 starts at slot 5 (second slot of block 1) and runs through the boundaries at 8, 12 and 16"""
    ids = np.array([1, 13, 2, 1,  1, 3, 4, 5,  6, 7, 8, 13,  9, 10, 6, 11,  12, 1, 2, 13], dtype=np.uint32)
    return ids, np.array([0, 5, 18, 20], dtype=np.uint64)


def test_mapping_carry_in_through_several_blocks(sim, dsim, tabs):
    ids, off = _carry_case()
    st = _check_csr(sim, dsim, tabs[1], ids, off, "carry", lanes=1)
    assert st["carries"] >= 4 and st["carry_reductions"] >= 3        # blocks 2, 3 and 4 all reach back to slot 5
    # the same with the start on a block's FIRST slot (no reduction: the scanned sum is the start sum) and on its LAST slot
    for start in (4, 7):
        o = np.array([0, start, 18, 20], dtype=np.uint64)
        st = _check_csr(sim, dsim, tabs[1], ids, o, ("carry", start), lanes=1)
        assert st["carry_reductions"] == (0 if start == 4 else 3)
    rng = np.random.default_rng(5113)
    for which in (0, 1):
        v = _ids(rng, which, 3000, 0.1)
        for o in ([0, 3000], [0, 1023, 3000], [0, 1024, 3000], [0, 1, 2999, 3000], [0, 700, 701, 2900, 3000]):
            _check_csr(sim, dsim, tabs[which], v, np.array(o, dtype=np.uint64), ("kernel geometry", o))


def test_mapping_empty_documents_and_zero_length_slots(sim, dsim, tabs):
    rng = np.random.default_rng(5114)
    pair = tabs[1]
    ids = _ids(rng, 1, 16, 0.0)
    # runs of empty documents across a block boundary (slot 8 with two lanes), at the start, trailing
    for off in ([0, 8] + [8] * 7 + [16], [0] * 6 + [16], [0, 16] + [16] * 9, [0, 7, 7, 7, 8, 8, 9, 16, 16], [0] * 4):
        _check_csr(sim, dsim, pair, ids if off[-1] else ids[:0], np.array(off, dtype=np.uint64), ("empties", off), lanes=2)
    # zero-length slots (the empty token, an unknown id, a skipped special) at a document's start and end, and a whole document of them
    z = np.array([0, 77, 3, 4, 20, 0,  77, 0, 20,  20, 4, 5, 1, 77], dtype=np.uint32)
    for flags in (0, SKIP_SPECIAL):
        for lanes in (1, 2, 3):
            _check_csr(sim, dsim, pair, z, np.array([0, 6, 9, 14], dtype=np.uint64), ("zero-length", flags, lanes), flags=flags, lanes=lanes)
    # the kernels' geometry: 5 000 empty documents in a run, in front, on the boundary at 1 024, trailing
    v = _ids(rng, 1, 2500)
    for name, off in {"first": [0] * 5000 + [1024, 2500], "boundary": [0, 1024] + [1024] * 5000 + [2500], "last": [0, 1000] + [2500] * 5000,
                      "slot": [0] + [700] * 300 + [701] * 300 + [2500]}.items():
        st = _check_csr(sim, dsim, pair, v, np.array(off, dtype=np.uint64), name)
        assert st["max_rounds"] >= 2 or len(off) < 5000, name
    _check_csr(sim, dsim, pair, _ids(rng, 1, 3000), np.arange(3001, dtype=np.uint64), "3 000 one-id documents")


def test_mapping_continuation_at_a_documents_first_token_and_three_way_splits(sim, dsim, tabs):
    pair = tabs[1]
    # 96 | e4 b8 | 96 | e7 95 8c ; then 🧑 ZWJ 🚀 in eight pieces, a document boundary INSIDE a character (slot 10)
    ids = np.array([4, 3, 4, 5, 6, 7, 8, 9, 10, 6, 11, 12], dtype=np.uint32)
    for lanes in (1, 2, 3):
        got = sim.spans(pair[1], ids, np.array([0, 4, 10, 12], dtype=np.uint64), lanes=lanes)
        assert got[1][:, 0].tolist() == [0, 0, 0, 1,  0, 0, 0, 1, 1, 2,  0, 0], lanes        # slots 0 and 10: cs == 0, the start stays 0
        assert got[1][:, 1].tolist() == [0, 1, 1, 2,  1, 1, 1, 2, 2, 3,  0, 0], lanes
        _check_csr(sim, dsim, pair, ids, np.array([0, 4, 10, 12], dtype=np.uint64), ("splits", lanes), lanes=lanes)


@pytest.mark.parametrize("row_len", [1, 7, 37, 65, 1024, 1025])
def test_mapping_rows(sim, dsim, tabs, row_len):
    rng = np.random.default_rng(row_len)
    n = {1: 2100, 7: 300, 37: 65, 65: 37, 1024: 3, 1025: 3}[row_len]
    for which in (0, 1):
        rows = _ids(rng, which, n * row_len, 0.2).astype(np.int64).reshape(n, row_len)      # padding slots hold ids that would decode
        lens = rng.integers(-2, row_len + 3, size=n).astype(np.int32)
        lens[0], lens[n - 1], lens[n // 2] = 0, row_len, row_len + 100
        odd = rows.copy()
        k = max(4, odd.size // 50)
        odd.flat[rng.integers(0, odd.size, size=k)] = rng.choice([-1, -100, 1 << 32, (1 << 32) + 4], size=k)
        for r, ln, flags in ((rows, None, I64), (rows, lens, I64), (rows, lens, I64 | PAD_LEFT), (odd, lens, I64 | PAD_LEFT | SKIP_SPECIAL),
                             (rows.astype(np.uint32), lens, 0), (rows.astype(np.uint32), lens, PAD_LEFT | SKIP_SPECIAL)):
            _check_rows(sim, dsim, tabs[which], r, ln, (row_len, which, flags), flags=flags, i64=bool(flags & PAD_LEFT))
    small = _ids(rng, 1, 5 * 7, 0.1).reshape(5, 7)
    for lanes in (1, 2, 3):
        for flags in (0, PAD_LEFT):
            _check_rows(sim, dsim, tabs[1], small, np.array([7, 0, 3, 9, -1], dtype=np.int32), (lanes, flags), flags=flags, lanes=lanes)


def test_mapping_offsets_that_claim_more_than_the_capacity(sim, dsim, tabs):
    rng = np.random.default_rng(5115)
    ids = _ids(rng, 1, 2048)
    off = _split(rng, 2048, 40)
    for n_cap in (2048, 2047, 1025, 1024, 1, 0):
        _check_csr(sim, dsim, tabs[1], ids, off, ("clamp", n_cap), n_cap=n_cap)
    _check_csr(sim, dsim, tabs[1], ids, off, "cap far above", poison_tail=9000)
    # slots between the clamped end and the capacity belong to no document: (0, 0)
    got = sim.spans(tabs[1][1], np.concatenate([ids[:10], np.full(30, 13, np.uint32)]), np.array([0, 4, 10], dtype=np.uint64), n_cap=40, lanes=2)
    assert not got[0][10:].any() and not got[1][10:].any() and got[0][:10].any()


@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, 2049])
def test_mapping_block_edges_at_the_kernels_geometry(sim, dsim, tabs, n):
    g = sim.geometry()
    assert g["block"] == 1024 and g["lanes"] * g["per_lane"] == g["block"] and g["max_token_bytes"] == 32767
    rng = np.random.default_rng(n)
    for which in (0, 1):
        ids = _ids(rng, which, n)
        for off in ([0, n], _split(rng, n, 9).tolist(), [0, min(1024, n), n]):
            for i64 in (False, True):
                st = _check_csr(sim, dsim, tabs[which], ids, np.array(off, dtype=np.uint64), (n, which, len(off), i64), i64=i64)
                assert st["blocks"] == n // 1024 + 1


def test_int32_entries_saturate_and_the_offsets_stay_exact(sim):
    """a table whose id 1 is 1.25 * 2^30 bytes long (no such byte string exists: spans read no text)"""
    HUGE = 5 << 28
    tab = decode_ref.Table({0: b"ab", 1: "é".encode(), 2: b"c"})
    st = sim.SpanTable(tab, 7, huge={1: HUGE})
    ids = np.array([0, 1, 0, 1,  1, 2, 0, 1,  2], dtype=np.uint32)
    off = np.array([0, 6, 9], dtype=np.uint64)
    stand_in = lambda i, ln, nch, cont: (HUGE if i == 1 else ln, nch, cont)
    for i64 in (False, True):
        got = sim.spans(st, ids, off, lanes=1, i64=i64)
        _same(got, ref.spans_csr(tab, ids, off, 9, 0, i64, length_of=stand_in), i64)
    b32 = sim.spans(st, ids, off, lanes=1)[0]
    assert b32[3].tolist() == [HUGE + 4, INT32_MAX] and b32[4].tolist() == [INT32_MAX, INT32_MAX] and b32[5].tolist() == [INT32_MAX, INT32_MAX]
    assert b32[6].tolist() == [0, 2] and b32[7].tolist() == [2, HUGE + 2]                 # the next document starts from 0 again
    got = sim.spans(st, ids, off, lanes=1, i64=True)
    assert got[0][5].tolist() == [3 * HUGE + 4, 3 * HUGE + 5] and got[2].tolist() == [0, 3 * HUGE + 5, 4 * HUGE + 8]


# ------------------------------------------------------------------------------------------ 4. two mutants, and the cases that catch them
def test_mutant_carry_in_from_the_blocks_base_is_caught(sim, dsim, tabs):
    """the start sums of the document that reaches into a block taken from the block's base: every slot of such a block restarts at 0.
    test_mapping_carry_in_through_several_blocks' first case and test_mapping_exhaustive_small_blocks fail with it."""
    ids, off = _carry_case()
    with pytest.raises(AssertionError, match="byte_span"):
        _check_csr(sim, dsim, tabs[1], ids, off, "carry", lanes=1, mutant=1)
    got = sim.spans(tabs[1][1], ids, off, lanes=1, mutant=1)
    assert got[0][8].tolist()[0] == 0 and ref.spans_csr(tabs[1][0], ids, off, 20)[0][8, 0] > 0
    assert got[2].tolist() == ref.spans_csr(tabs[1][0], ids, off, 20)[2].tolist()            # (the offsets do not depend on it)
    # a document that starts on its block's first slot and ends inside it needs no carry-in: such a case cannot tell
    _check_csr(sim, dsim, tabs[1], ids[:8], np.array([0, 4, 8], dtype=np.uint64), "no carry", lanes=1, mutant=1)


def test_mutant_dropped_continuation_adjustment_is_caught(sim, dsim, tabs):
    """the character start not moved back for a token that begins inside a character: the pinned tiktoken starts and
    test_mapping_continuation_at_a_documents_first_token_and_three_way_splits fail with it; the byte spans and a first token that begins
    with a continuation byte (cs == 0) do not depend on it."""
    for text, lens, starts in PINNED:
        pieces = _pieces(text, lens)
        tab = decode_ref.Table(dict(enumerate(pieces)))
        st = sim.SpanTable(tab, len(pieces) + 2)
        ids = np.arange(len(pieces), dtype=np.uint32)
        got = sim.spans(st, ids, np.array([0, len(ids)], dtype=np.uint64), lanes=2, mutant=2)
        assert got[1][:, 0].tolist() != starts, text
        assert np.array_equal(got[0], ref.spans_csr(tab, ids, [0, len(ids)], len(ids))[0])
    with pytest.raises(AssertionError, match="char_span"):
        _check_csr(sim, dsim, tabs[1], np.array([4, 3, 4, 5], dtype=np.uint32), np.array([0, 4], dtype=np.uint64), "cont", lanes=1, mutant=2)
    _check_csr(sim, dsim, tabs[1], np.array([4, 1, 2, 5], dtype=np.uint32), np.array([0, 1, 4], dtype=np.uint64), "cont at cs == 0 only", lanes=1, mutant=2)
