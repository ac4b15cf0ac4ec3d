"""spl_decode_batch_device without a GPU: the C ABI's symbols, struct and refusals, the Python surface's ValueErrors, tests/decode_ref.py
against examples written out by hand, and the mapping code the kernels run (splintr_amd/csrc/spl_k_decode_dev.h, evaluated block by
block and lane by lane by tests/hostsim/decode_sim.cpp) against decode_ref on a synthetic table with token lengths 0, 1, 2, 3, 4, 5,
15, 16, 17, 255 and 300."""
import ctypes
import os
import re

import numpy as np
import pytest

import decode_ref as ref
from decode_ref import I64, PAD_LEFT, SKIP_SPECIAL
from conftest import ROOT

SPL_EINVAL = -1


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as entry
    entry.build()
    from splintr_amd import _ffi
    return _ffi


@pytest.fixture(scope="module")
def sim():
    import decode_sim
    decode_sim.lib()
    return decode_sim


@pytest.fixture(scope="module")
def tab():
    return ref.synthetic_table()


@pytest.fixture(scope="module")
def dtab(sim, tab):
    return sim.DeviceTable(tab, ref.SYN_MAX_ID)


# ------------------------------------------------------------------------------------------ 1. the C ABI
def test_symbols_and_struct_layout(ffi):
    L = ffi.lib()
    for s in ("spl_decode_reserve_device", "spl_decode_batch_device", "spl_max_token_bytes"):
        assert hasattr(L, s) and s in ffi.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "splintr_hip.h")).read()
    body = re.search(r"typedef struct spl_decode_opts \{(.*?)\} spl_decode_opts;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip() for decl in re.findall(r"uint32_t ([^;]+);", body) for n in decl.split(",")]
    assert fields == ["struct_size", "flags", "row_len"]
    O = ffi.SplDecodeOpts
    assert [f[0] for f in O._fields_] == fields and all(f[1] is ctypes.c_uint32 for f in O._fields_)
    assert ctypes.sizeof(O) == 12 and [getattr(O, f).offset for f in fields] == [0, 4, 8]
    assert O(3, 5).struct_size == 12 and O(3, 5).flags == 3 and O(3, 5).row_len == 5
    for name, val in (("I64", 1), ("PAD_LEFT", 2), ("SKIP_SPECIAL", 4)):
        assert re.search(r"#define SPL_DECODE_%s\s+%du\b" % (name, val), hdr), name
        assert getattr(ffi, "SPL_DECODE_" + name) == val
    assert L.spl_max_token_bytes(None) == 0


def test_refusals_name_their_cause(ffi):
    """Every refusal comes before the handle or the device is touched: a dummy handle (never read) is enough, and none of the addresses
    below is ever dereferenced."""
    L = ffi.lib()
    handle = ctypes.create_string_buffer(64)
    h = ctypes.addressof(handle)
    A = 0x10000                       # an address that is aligned to everything
    O = ffi.SplDecodeOpts
    NIL = "nil"

    def call(t=h, ids=A, cap=100, off=NIL, ln=None, n=3, o=None, out=A, bcap=64, oo=A):
        o = O(0, 0) if o is None else o
        if off is NIL:
            off = None if (o is not False and o.row_len) else A
        return L.spl_decode_batch_device(t, ids, cap, off, ln, n, ctypes.byref(o) if o is not False else None, out, bcap, oo, None)

    def refused(rc, *words):
        msg = L.spl_last_error().decode()
        assert rc == SPL_EINVAL, (rc, msg)
        for w in ("spl_decode_batch_device",) + words:
            assert w in msg, (w, msg)

    refused(call(t=None), "null handle")
    refused(call(o=False), "options")
    refused(call(oo=None), "d_out_off is null")
    refused(call(ids=None), "d_ids is null")
    refused(call(ids=None, o=O(0, 8)), "d_ids is null")
    refused(call(out=None), "d_bytes is null", "bytes_capacity")
    short = O(0, 0)
    short.struct_size = 0
    refused(call(o=short), "struct_size")
    short.struct_size = 8
    refused(call(o=short), "struct_size")
    short.struct_size = 4097
    refused(call(o=short), "struct_size")
    refused(call(o=O(8, 0)), "unknown flag bit 0x8")
    refused(call(o=O(0x80000000 | I64, 4)), "unknown flag bit 0x80000000")
    refused(call(o=O(PAD_LEFT, 0)), "SPL_DECODE_PAD_LEFT", "CSR mode")
    refused(call(ln=A), "d_len", "CSR mode")
    refused(call(off=None), "d_ids_off is null", "CSR mode")
    refused(call(o=O(0, 8), off=A), "d_ids_off", "rows mode")
    refused(call(out=A + 8), "d_bytes", "16-byte")
    refused(call(ids=A + 4), "d_ids", "16-byte")
    refused(call(ids=A + 16, o=O(I64, 0)), "d_ids", "32-byte")
    refused(call(ids=A + 16, o=O(I64, 7)), "d_ids", "32-byte")
    refused(call(n=1 << 31), "n_docs >= 2^31")
    refused(call(cap=1 << 41), "n_ids_cap", "2^41")
    refused(call(n=1 << 30, o=O(0, 1 << 11)), "n_docs * row_len", "2^41")
    # a LONGER struct is accepted and its tail ignored: the refusal that follows is about something else
    big = (ctypes.c_uint32 * 16)(64, 0, 0, 0xFFFFFFFF, 0xFFFFFFFF)
    refused(call(o=ctypes.cast(big, ctypes.POINTER(O)).contents, off=None), "d_ids_off is null")
    assert "struct_size" not in L.spl_last_error().decode()
    # the reserve call
    assert L.spl_decode_reserve_device(None, 10) == SPL_EINVAL and "null handle" in L.spl_last_error().decode()
    assert L.spl_decode_reserve_device(h, 1 << 41) == SPL_EINVAL and "2^41" in L.spl_last_error().decode()


def test_python_surface_validates_before_anything_goes_to_the_device():
    """A bad dtype, rank, device, layout, side string or size raises ValueError before the handle is used: a tokenizer object without
    one is enough to see it (a CPU tensor is refused as such -- device-resident decode takes no host tensor)."""
    import torch
    from splintr_amd import Tokenizer
    from splintr_amd import device as dv
    t = Tokenizer.__new__(Tokenizer)
    rows = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(ValueError, match="errors"):
        t.decode_tensor(rows, errors="ignore")
    with pytest.raises(ValueError, match="padding_side"):
        t.decode_tensor(rows, padding_side="up")
    with pytest.raises(ValueError, match="dtype"):
        t.decode_tensor(rows.to(torch.int16))
    with pytest.raises(ValueError, match="dtype"):
        t.decode_tensor([[1, 2, 3]])
    with pytest.raises(ValueError, match="on a GPU"):
        t.decode_tensor(rows)
    with pytest.raises(ValueError, match="on a GPU"):
        dv.decode_rows_device(t, rows, max_bytes=16)
    with pytest.raises(ValueError, match="on a GPU"):
        dv.decode_device(t, rows.flatten(), torch.zeros(2, dtype=torch.int64), max_bytes=16)
    with pytest.raises(ValueError, match="max_bytes"):
        dv.decode_rows_device(t, rows, max_bytes=-1)
    with pytest.raises(ValueError, match="max_bytes"):
        dv.decode_device(t, rows.flatten(), torch.zeros(2, dtype=torch.int64), max_bytes=1.5)
    with pytest.raises(ValueError, match="padding_side"):
        dv.decode_rows_device(t, rows, max_bytes=16, padding_side="middle")
    # rank, layout and the companions' shapes come before the device: host tensors are enough to see them
    chk = dv.check_decode_args
    m = torch.zeros((4, 6), dtype=torch.int32)
    with pytest.raises(ValueError, match="rank 2"):
        chk(m.flatten(), rows=True)
    with pytest.raises(ValueError, match="rank 1"):
        chk(m, torch.zeros(3, dtype=torch.int64), rows=False)
    with pytest.raises(ValueError, match="contiguous"):
        chk(m.t(), rows=True)
    with pytest.raises(ValueError, match="lengths"):
        chk(m, None, torch.zeros(4, dtype=torch.int64), rows=True)
    with pytest.raises(ValueError, match="lengths"):
        chk(m, None, torch.zeros(5, dtype=torch.int32), rows=True)
    with pytest.raises(ValueError, match="offsets"):
        chk(m.flatten(), torch.zeros(3, dtype=torch.int32), rows=False)
    with pytest.raises(ValueError, match="offsets"):
        chk(m.flatten(), None, rows=False)
    with pytest.raises(ValueError, match="on a GPU"):                      # (everything else is in order)
        chk(m, None, torch.zeros(4, dtype=torch.int32), rows=True, max_bytes=5)


# ------------------------------------------------------------------------------------------ 2. decode_ref against hand-written examples
def _tiny():
    return ref.Table({1: b"a", 2: b"bc", 5: b"<s>", 7: b"xyz", 9: b"", 4000000000: b"<far>"}, special_only={5, 4000000000})


def test_ref_csr_by_hand():
    t = _tiny()
    ids = [1, 3, 2, 5, 7, 4000000000, 1, 1]              # 3 is a hole
    raw, off, need = ref.decode_csr(t, ids, [0, 3, 3, 6, 7], 8)
    assert raw == b"abc" + b"<s>xyz<far>" + b"a" and off.tolist() == [0, 3, 3, 14, 15] and need == 15
    raw, off, need = ref.decode_csr(t, ids, [0, 3, 3, 6, 7], 8, SKIP_SPECIAL)
    assert raw == b"abc" + b"xyz" + b"a" and off.tolist() == [0, 3, 3, 6, 7]
    # the CSR claims more than n_ids_cap = 4: every offset is clamped; document 2 keeps only id 5, document 3 is empty
    raw, off, need = ref.decode_csr(t, ids, [0, 3, 3, 6, 7], 4)
    assert raw == b"abc<s>" and off.tolist() == [0, 3, 3, 6, 6] and need == 6
    # the capacity cuts the bytes, never the offsets
    raw, off, need = ref.decode_csr(t, ids, [0, 3, 3, 6, 7], 8, 0, capacity=5)
    assert raw == b"abc<s" and off.tolist() == [0, 3, 3, 14, 15] and need == 15


def test_ref_rows_by_hand():
    t = _tiny()
    rows = np.array([[1, 2, 7], [7, 2, 1], [5, 1, 5]], dtype=np.int64)
    assert ref.decode_rows(t, rows, None, I64)[0] == b"abcxyz" + b"xyzbca" + b"<s>a<s>"
    raw, off, _ = ref.decode_rows(t, rows, [2, 0, 9], I64)                 # 9 is clamped to 3
    assert raw == b"abc" + b"" + b"<s>a<s>" and off.tolist() == [0, 3, 3, 10]
    raw, off, _ = ref.decode_rows(t, rows, [2, -4, 1], I64 | PAD_LEFT)     # the LAST entries; -4 is clamped to 0
    assert raw == b"bcxyz" + b"" + b"<s>" and off.tolist() == [0, 5, 5, 8]
    raw, off, _ = ref.decode_rows(t, rows, [2, -4, 1], I64 | PAD_LEFT | SKIP_SPECIAL)
    assert raw == b"bcxyz" and off.tolist() == [0, 5, 5, 5]


def test_ref_int64_values_outside_32_bits_are_no_ids():
    t = _tiny()
    rows = np.array([[-1, 1, -100, (1 << 32) + 1, 1 << 32, 2]], dtype=np.int64)
    assert ref.decode_rows(t, rows, None, I64)[0] == b"abc"
    # the same 32-bit patterns WITHOUT the flag are ids: 0xFFFFFFFF and 0xFFFFFF9C are unknown, 4000000000 is the far special
    ids = np.array([0xFFFFFFFF, 1, 0xFFFFFF9C, 4000000000], dtype=np.uint32)
    assert ref.decode_csr(t, ids, [0, 4], 4)[0] == b"a<far>"
    assert ref.decode_csr(t, ids.view(np.int32), [0, 4], 4)[0] == b"a<far>"       # int32 input is read as the 32-bit pattern


# ------------------------------------------------------------------------------------------ 3. the mapping code the kernels run
def _check_csr(sim, tab, dtab, ids, off, tag, *, n_cap=None, flags=0, capacity=None, lanes=None, poison_tail=0):
    """ids: the real ids (numpy); poison_tail more ids that WOULD decode to something are appended behind them (never to be read as part
    of a document); n_cap defaults to the length with the tail"""
    ids = np.asarray(ids)
    full = np.concatenate([ids, np.full(poison_tail, 10, dtype=ids.dtype)]) if poison_tail else ids
    n_cap = len(full) if n_cap is None else n_cap
    w_raw, w_off, need = ref.decode_csr(tab, full, off, n_cap, flags)
    cap = need if capacity is None else capacity
    raw, o, st = sim.decode(dtab, full, off, n_cap=n_cap, flags=flags, capacity=cap, lanes=lanes)
    assert o.tolist() == w_off.tolist(), tag
    assert raw == w_raw[:min(need, cap)], tag
    return st, need


def _split(rng, n, n_docs):
    """n ids into n_docs documents, empty ones among them"""
    cuts = np.sort(rng.integers(0, n + 1, size=max(n_docs - 1, 0)))
    return np.concatenate([[0], cuts, [n]]).astype(np.uint64) if n_docs else np.zeros(1, dtype=np.uint64)


def test_mapping_exhaustive_small_blocks(sim, tab, dtab):
    """Every id count 0 .. 40 with workgroups of 1, 2 and 3 lanes (blocks of 4, 8 and 12 slots): every block edge, the end at a multiple of
    the block, zero-byte blocks, documents that share slots -- with unknown ids in front of tokens everywhere (p_unknown)."""
    rng = np.random.default_rng(4111)
    cases = 0
    for lanes in (1, 2, 3):
        for n in range(41):
            for rep in range(3):
                ids = ref.random_ids(rng, n, p_unknown=(0.25, 0.6, 0.0)[rep])
                off = _split(rng, n, int(rng.integers(0, 7)))
                for flags in (0, SKIP_SPECIAL):
                    _check_csr(sim, tab, dtab, ids, off, (lanes, n, rep, flags, ids.tolist(), off.tolist()), flags=flags, lanes=lanes)
                    cases += 1
                # an upper bound far above the count, and a clamp below it (the ids beyond are poison that would decode to something)
                _check_csr(sim, tab, dtab, ids, off, (lanes, n, "tail"), lanes=lanes, poison_tail=int(rng.integers(1, 30)))
                if n:
                    _check_csr(sim, tab, dtab, ids, off, (lanes, n, "clamp"), lanes=lanes, n_cap=int(rng.integers(0, n)))
                i64 = ids.astype(np.int64)
                if n:
                    i64[int(rng.integers(n))] = (-1, -100, 1 << 32, (1 << 32) + 4)[rep + (n & 1)]
                _check_csr(sim, tab, dtab, i64, off, (lanes, n, "i64", i64.tolist()), flags=I64, lanes=lanes)
    assert cases > 700


def test_mapping_every_capacity(sim, tab, dtab):
    """capacity 0 .. need + 1 on a small case: cuts inside a token, inside a group, at a group's edge and at a block's edge"""
    rng = np.random.default_rng(4112)
    ids = np.array([4, 12, 8, 1, 1, 7, 19, 2, 5, 6, 3, 20, 100300, 9, 4, 1], dtype=np.uint32)        # 12 and 19 are holes; 9 is 255 bytes
    off = np.array([0, 0, 3, 3, 9, 16, 16], dtype=np.uint64)
    need = ref.decode_csr(tab, ids, off, len(ids))[2]
    assert need > 300
    for lanes in (1, 2, 256):
        for cap in range(need + 2):
            _check_csr(sim, tab, dtab, ids, off, (lanes, cap), capacity=cap, lanes=lanes)
    del rng


def _block_case(rng, n, kind):
    if kind == "ones":
        return np.full(n, 1, dtype=np.uint32)                    # single-byte tokens only
    if kind == "long":
        return np.full(n, 10, dtype=np.uint32)                   # the 300-byte token: one block is 307 200 bytes
    return ref.random_ids(rng, n)


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2048, 2049, 3073])
def test_mapping_block_edges_at_the_kernels_geometry(sim, tab, dtab, n):
    g = sim.geometry()
    assert g["block"] == 1024 and g["lanes"] * g["per_lane"] == g["block"] and g["group"] in (4, 16)
    rng = np.random.default_rng(n)
    for kind in ("mixed", "ones", "long"):
        ids = _block_case(rng, n, kind)
        for off in (np.array([0, n], dtype=np.uint64), _split(rng, n, 9),
                    np.array([0, min(1024, n), n], dtype=np.uint64)):                     # a boundary exactly at slot 1 024
            st, need = _check_csr(sim, tab, dtab, ids, off, (n, kind, len(off)))
            assert st["wide"] > 0 and st["blocks"] == n // 1024 + 1
    # block sums of chosen residues: the first block's byte count is 1, 2, 3 (mod 4) and 1, 15 (mod 16) -- its range ends one byte into a
    # 16-byte group, or one byte short of one, and the next block's starts there.  Four-byte tokens, ONE token of n_odd bytes and k unknown ids
    # (in front of tokens), k chosen so that 4 * (slots - 1 - k) + n_odd has the wanted residue; asserted from the reference.
    first = min(n, 1024)
    odd_id = {1: 1, 2: 2, 3: 3, 15: 6, 17: 8}
    for n_odd, want16 in ((1, 1), (15, 15), (17, 1), (2, 2), (3, 3), (3, 15), (1, 13)):
        k = next(k for k in range(1, 6) if (4 * (first - 1 - k) + n_odd) % 16 == want16)
        ids = np.full(n, 4, dtype=np.uint32)
        ids[5] = odd_id[n_odd]
        ids[[700, 300, 900, 100, 500][:k]] = 12
        block_sum = ref.decode_csr(tab, ids[:first], [0, first], first)[2]
        assert block_sum % 16 == want16 and block_sum % 4 == n_odd % 4 != 0, (n, n_odd, want16, block_sum)
        _check_csr(sim, tab, dtab, ids, np.array([0, 5, n], dtype=np.uint64), (n, "residue", n_odd, want16))
    # a block of 1 024 unknown ids (zero bytes) between two ordinary blocks, first, and last
    for where in ("between", "first", "last"):
        parts = {"between": [ref.random_ids(rng, 1024, 0.1), np.full(1024, 77, np.uint32), ref.random_ids(rng, n % 1024 + 1, 0.1)],
                 "first": [np.full(1024, 77, np.uint32), ref.random_ids(rng, 1025, 0.1)],
                 "last": [ref.random_ids(rng, 1024, 0.1), np.full(1024, 0xFFFFFFFF, np.uint32)]}[where]
        ids = np.concatenate(parts)
        _check_csr(sim, tab, dtab, ids, _split(rng, len(ids), 5), (n, "zero block", where))


def test_mapping_documents(sim, tab, dtab):
    rng = np.random.default_rng(4113)
    z = np.zeros(0, dtype=np.uint32)
    _check_csr(sim, tab, dtab, z, [0], "no document")
    _check_csr(sim, tab, dtab, z, [0, 0, 0, 0], "three empty documents, no id")
    ids = ref.random_ids(rng, 2500)
    runs = {"first": [0] * 5000 + [1024, 2500], "boundary": [0, 1024] + [1024] * 5000 + [2500], "last": [0, 1000] + [2500] * 5000,
            "three blocks": [0, 10, 2300, 2500], "slot": [0] + [700] * 300 + [701] * 300 + [2500]}
    for name, off in runs.items():
        st, _ = _check_csr(sim, tab, dtab, ids, np.array(off, dtype=np.uint64), name)
        if len(off) > 5000:
            assert st["max_rounds"] >= 2, name                   # the cooperative search needs a second round
    ones = np.arange(3001, dtype=np.uint64)
    _check_csr(sim, tab, dtab, ref.random_ids(rng, 3000), ones, "3 000 one-id documents")
    # n_ids_cap: equal to the count, far above it, a multiple of 1 024 equal to the count, below the count
    ids = ref.random_ids(rng, 2048)
    off = _split(rng, 2048, 40)
    _check_csr(sim, tab, dtab, ids, off, "cap == count == 2 * 1024")
    _check_csr(sim, tab, dtab, ids, off, "cap far above", poison_tail=9000)
    for n_cap in (2047, 1025, 1024, 1, 0):
        _check_csr(sim, tab, dtab, ids, off, ("clamp", n_cap), n_cap=n_cap)


@pytest.mark.parametrize("row_len", [1, 7, 1024, 1025])
def test_mapping_rows(sim, tab, dtab, row_len):
    rng = np.random.default_rng(row_len)
    n = {1: 2100, 7: 300, 1024: 3, 1025: 3}[row_len]
    rows = ref.random_ids(rng, n * row_len, 0.2).astype(np.int64).reshape(n, row_len)     # padding slots hold ids that would decode to something
    lens = rng.integers(-2, row_len + 3, size=n).astype(np.int32)
    lens[0], lens[n - 1], lens[n // 2] = 0, row_len, row_len + 100
    odd = rows.copy()
    odd.flat[rng.integers(0, odd.size, size=max(4, odd.size // 50))] = rng.choice([-1, -100, 1 << 32, (1 << 32) + 17], size=max(4, odd.size // 50))
    for r, ln, flags in ((rows, None, I64), (rows, lens, I64), (rows, lens, I64 | PAD_LEFT), (odd, lens, I64 | PAD_LEFT | SKIP_SPECIAL),
                         (odd, None, I64), (rows.astype(np.uint32), lens, 0), (rows.astype(np.uint32), lens, PAD_LEFT | SKIP_SPECIAL)):
        w_raw, w_off, need = ref.decode_rows(tab, r, ln, flags)
        for cap in (need, max(need - 1, 0), need // 2):
            raw, o, st = sim.decode(dtab, r, None, ln, row_len=row_len, flags=flags, capacity=cap)
            assert o.tolist() == w_off.tolist(), (row_len, flags, cap)
            assert raw == w_raw[:min(need, cap)], (row_len, flags, cap)
    # (2^32 + 17 must not alias id 17 -- which is unknown here; 2^32 + 4 would alias the 4-byte token)
    r = np.full((1, row_len), (1 << 32) + 4, dtype=np.int64)
    assert sim.decode(dtab, r, None, None, row_len=row_len, flags=I64, capacity=16)[0] == b""
