"""spl_pair_device without a GPU: the C ABI's refusals, the mapping code the kernel runs (splintr_amd/csrc/spl_k_pair.h, evaluated for
every output element by tests/hostsim/pair_sim.cpp) against tests/pair_ref.py, the kernel's closed form of LONGEST_FIRST against the
sequential rule, and pair_ref against examples written out by hand."""
import ctypes
import os
import re

import numpy as np
import pytest

import pair_ref as ref
from pair_ref import I64, KEEP_TAIL_A, KEEP_TAIL_B, LONGEST_FIRST, ONLY_FIRST, ONLY_SECOND, PAD_LEFT
from conftest import ROOT

SPL_EINVAL = -1
PAD_ID = 0xFFFFFFFF


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as entry
    entry.build()
    from splintr_amd import _ffi
    return _ffi


@pytest.fixture(scope="module")
def sim():
    import pair_sim
    pair_sim.lib()
    return pair_sim


# ------------------------------------------------------------------------------------------ 1. the C ABI
def test_symbol_and_struct_layout(ffi):
    L = ffi.lib()
    assert hasattr(L, "spl_pair_device") and "spl_pair_device" in ffi.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "splintr_hip.h")).read()
    body = re.search(r"typedef struct spl_pair_opts \{(.*?)\} spl_pair_opts;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip() for decl in re.findall(r"uint32_t ([^;]+);", body) for n in decl.split(",")]
    assert fields == ["struct_size", "flags", "row_len", "pad_id", "trunc", "n_prefix", "n_middle", "n_suffix", "prefix[32]", "middle[32]",
                      "suffix[32]"]
    O = ffi.SplPairOpts
    names = [f[0] for f in O._fields_]
    assert names == [f.split("[")[0] for f in fields]
    assert all(f[1] is ctypes.c_uint32 for f in O._fields_[:8]) and all(f[1] is ctypes.c_uint32 * 32 for f in O._fields_[8:])
    assert ctypes.sizeof(O) == 416
    assert [getattr(O, n).offset for n in names] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 160, 288]
    o = O(3, 5, 7, 2, prefix=(1,), middle=(2, 3), suffix=())
    assert (o.struct_size, o.flags, o.row_len, o.pad_id, o.trunc, o.n_prefix, o.n_middle, o.n_suffix) == (416, 3, 5, 7, 2, 1, 2, 0)
    assert o.prefix[0] == 1 and list(o.middle[:2]) == [2, 3]
    for name, val in (("MAX_FIXED", 32), ("KEEP_TAIL_A", 32), ("KEEP_TAIL_B", 64), ("LONGEST_FIRST", 0), ("ONLY_FIRST", 1), ("ONLY_SECOND", 2)):
        assert re.search(r"#define SPL_PAIR_%s\s+%du\b" % (name, val), hdr), name
        assert getattr(ffi, "SPL_PAIR_" + name) == val
    sig = re.search(r"int spl_pair_device\((.*?)\);", hdr, re.S).group(1)
    assert len(re.sub(r"/\*.*?\*/", "", sig, flags=re.S).split(",")) == len(L.spl_pair_device.argtypes) == 19


def test_refusals_name_their_cause(ffi):
    """Every refusal comes before the handle or the device is touched: a dummy handle (never read) is enough, and none of the addresses
    below is ever dereferenced."""
    L = ffi.lib()
    handle = ctypes.create_string_buffer(64)
    h = ctypes.addressof(handle)
    A = 0x10000                       # an address that is aligned to everything
    O = ffi.SplPairOpts

    def call(t=h, a_ids=A, a_off=A, n_a=3, b_ids=A, b_off=A, n_b=3, a_idx=None, b_idx=None, n=3, o=None, rows=A, mask=A, ty=A, sp=A, ln=A,
             kept=A, status=A):
        o = O(0, 8) if o is None else o
        return L.spl_pair_device(t, a_ids, a_off, n_a, b_ids, b_off, n_b, a_idx, b_idx, n, ctypes.byref(o) if o is not False else None,
                                 rows, mask, ty, sp, ln, kept, status, None)

    def refused(rc, *words):
        msg = L.spl_last_error().decode()
        assert rc == SPL_EINVAL, (rc, msg)
        for w in ("spl_pair_device",) + words:
            assert w in msg, (w, msg)

    refused(call(t=None), "null handle")
    refused(call(o=False), "options")
    refused(call(rows=None), "d_rows is null")
    refused(call(n=0, rows=None), "d_rows is null")
    refused(call(a_off=None), "d_a_off is null")
    refused(call(b_off=None), "d_b_off is null")
    refused(call(status=None), "d_status is null")
    refused(call(a_ids=None), "d_a_ids is null")
    refused(call(b_ids=None), "d_b_ids is null")
    short = O(0, 8)
    short.struct_size = 0
    refused(call(o=short), "struct_size")
    short.struct_size = 412
    refused(call(o=short), "struct_size")
    short.struct_size = 4097
    refused(call(o=short), "struct_size")
    refused(call(o=O(128, 8)), "unknown flag bit 0x80")
    refused(call(o=O(0x80000000 | PAD_LEFT, 8)), "unknown flag bit 0x80000000")
    for bit in (4, 8, 16):             # SPL_COLLATE_KEEP_TAIL, _BOS, _EOS
        refused(call(o=O(bit, 8)), "fixed segments", "SPL_PAIR_KEEP_TAIL_A")
    refused(call(o=O(0, 8, 0, 3)), "trunc")
    for seg in ("prefix", "middle", "suffix"):
        o = O(0, 200)
        setattr(o, "n_" + seg, 33)
        refused(call(o=o), "SPL_PAIR_MAX_FIXED")
    refused(call(o=O(0, 0)), "row_len is 0")
    refused(call(o=O(0, 2, prefix=(1,), middle=(2,), suffix=(3,))), "row_len", "fixed segments")
    refused(call(n_a=1 << 31, a_idx=A), "n_a >= 2^31")
    refused(call(n_b=1 << 31, b_idx=A), "n_b >= 2^31")
    refused(call(n=1 << 31, a_idx=A, b_idx=A), "n_pairs >= 2^31")
    refused(call(n=4), "d_a_idx is null", "n_a")
    refused(call(n=4, a_idx=A), "d_b_idx is null", "n_b")
    refused(call(n=(1 << 31) - 1, a_idx=A, b_idx=A, o=O(0, 0xFFFFFFFF), rows=A + 8), "d_rows", "16-byte")   # (n_pairs * row_len < 2^63: never refused for its size)
    refused(call(rows=A + 8), "d_rows", "16-byte")
    refused(call(ln=A + 4), "d_len", "16-byte")
    refused(call(kept=A + 8), "d_kept", "16-byte")
    refused(call(mask=A + 2), "d_mask", "4-byte")
    refused(call(ty=A + 1), "d_type", "4-byte")
    refused(call(sp=A + 3), "d_special", "4-byte")
    refused(call(a_idx=A + 2), "d_a_idx", "4-byte")
    refused(call(b_idx=A + 1), "d_b_idx", "4-byte")
    # a LONGER struct is accepted and its tail ignored: the refusal that follows is about something else
    big = (ctypes.c_uint32 * 200)(800, 0, 0)
    refused(call(o=ctypes.cast(big, ctypes.POINTER(O)).contents), "row_len is 0")
    assert "struct_size" not in L.spl_last_error().decode()
    # nothing to do is not an error, and needs no ids and no optional output
    assert call(n=0, a_ids=None, b_ids=None, mask=None, ty=None, sp=None, ln=None, kept=None) == 0


# ------------------------------------------------------------------------------------------ 2. the truncation rule
def test_closed_form_equals_the_sequential_rule(sim):
    """the kernel's cpair_trunc against Hugging Face's rule played one id at a time, for every (la, lb, B) in 0..12 cubed and every mode"""
    n = 0
    for mode in (LONGEST_FIRST, ONLY_FIRST, ONLY_SECOND):
        for la in range(13):
            for lb in range(13):
                for B in range(13):
                    got, want = sim.trunc(la, lb, B, mode), ref.truncate(la, lb, B, mode)
                    assert got == want, (mode, la, lb, B, got, want)
                    assert sum(got) == min(la + lb, B) and got[0] <= la and got[1] <= lb
                    n += 1
    assert n == 3 * 13 ** 3
    # lengths beyond 32 bits: the budget still decides
    assert sim.trunc(1 << 40, 3, 10, LONGEST_FIRST) == (7, 3) and sim.trunc(3, 1 << 40, 10, LONGEST_FIRST) == (3, 7)
    assert sim.trunc(1 << 40, 1 << 41, 11, LONGEST_FIRST) == (6, 5) and sim.trunc(1 << 40, 1 << 41, 11, ONLY_FIRST) == (0, 11)


# ------------------------------------------------------------------------------------------ 3. the mapping code the kernel runs
def _ids32(a):
    return (a & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def _compare(sim, src, a_idx, b_idx, n_pairs, L, flags, trunc, segs, tag, null=()):
    a_ids, a_off, n_a, b_ids, b_off, n_b = src
    want = ref.pair_ref(a_ids, a_off, n_a, b_ids, b_off, n_b, a_idx, b_idx, n_pairs, L, flags, PAD_ID, trunc, *segs)
    got = sim.pair(a_ids, a_off, n_a, b_ids, b_off, n_b, a_idx, b_idx, n_pairs, L, flags, PAD_ID, trunc, *segs, null=null)
    assert np.array_equal(got[0], _ids32(want[0])), tag
    for i, name in ((1, "mask"), (2, "type"), (3, "special"), (4, "len"), (5, "kept")):
        assert got[i] is None if name in null else np.array_equal(got[i], want[i]), (name,) + tag
    assert got[6] == want[6], tag
    return want


def test_pair_mapping_exhaustive(sim):
    cases, seen, residues = 0, set(), set()
    for L in ref.ROW_LENS + ref.LONG_ROW_LENS:
        for src, calls, _, flags, trunc, segs in ref.grid(L, 20260 + L):
            for kind, a_idx, b_idx, bad, n_pairs in calls:
                tag = (L, segs, trunc, flags, kind, n_pairs, src[1].tolist(), src[4].tolist())
                want = _compare(sim, src, a_idx, b_idx, n_pairs, L, flags, trunc, segs, tag)
                assert want[6] == (1 if bad else 0), tag
                residues.add((L, n_pairs * L % 4))
                seen.add((kind, trunc))
                seen.add(tuple(map(len, segs)))
                cases += 1
    assert cases > 5000
    for L in ref.ROW_LENS:
        assert {r for (l, r) in residues if l == L} == ({0, 1, 2, 3} if L % 2 else {0, 2} if L % 4 else {0}), L
    assert all((kind, trunc) in seen for kind in ref.KINDS for trunc in (0, 1, 2))
    assert all(c in seen for c in ((0, 0, 0), (1, 1, 1), (1, 2, 1), (32, 32, 32), (9, 0, 0), (32, 32, 1)))     # (the last two: k == row_len at 9 and 65)


def test_pair_mapping_optional_outputs_and_more_than_one_workgroup(sim):
    """each optional output as NULL once; a few thousand pairs: more than one span, rows that straddle lanes and workgroups"""
    rng = np.random.default_rng(20261)
    g = sim.geometry()
    segs = ((0xA0000000,), (0xB0000000, 0xB0000001), (0xC0000000,))
    for n_docs, L in ((300, 65), (1025, 3), (2100, 5), (700, 64)):
        budget = L - 4 if L >= 4 else L
        sg = segs if L >= 4 else ((), (), ())
        a_ids, a_off = ref.csr(ref.sweep_lengths(budget, n_docs, rng), rng)
        b_ids, b_off = ref.csr(ref.sweep_lengths(budget, n_docs, rng), rng)
        assert n_docs * L > g["span"]
        src = (a_ids, a_off, n_docs, b_ids, b_off, n_docs)
        _compare(sim, src, None, None, n_docs, L, PAD_LEFT | KEEP_TAIL_B, LONGEST_FIRST, sg, (n_docs, L, "identity"))
        a_idx = [int(x) for x in rng.integers(0, n_docs, size=n_docs + 3)]
        _compare(sim, src, a_idx, [0] * (n_docs + 3), n_docs + 3, L, KEEP_TAIL_A, ONLY_SECOND, sg, (n_docs, L, "indexed"))
    for name in ("mask", "type", "special", "len", "kept"):
        _compare(sim, src, None, None, 257, L, 0, LONGEST_FIRST, sg, ("null", name), null=(name,))
    _compare(sim, src, None, None, 257, L, 0, LONGEST_FIRST, sg, ("null", "all"), null=("mask", "type", "special", "len", "kept"))


def test_two_slices_of_one_csr(sim):
    """off[0] != 0: the two sides are the documents 0 .. n_a - 1 and n_a .. n_a + n_b - 1 of ONE encode result"""
    rng = np.random.default_rng(20262)
    n_a, n_b = 6, 8
    for L, segs in ((7, ((1,), (2,), (3,))), (64, ((), (9, 9), ())), (5, ((), (), ()))):
        k = sum(map(len, segs))
        ids, off = ref.csr(ref.sweep_lengths(L - k, n_a, rng) + ref.sweep_lengths(L - k, n_b, rng), rng)
        if int(off[n_a]) == 0:
            continue
        docs = [ids[int(off[i]):int(off[i + 1])].tolist() for i in range(n_a + n_b)]
        a_idx, b_idx = [5, 0, 1, 2, 3, 4, 4], [7, 6, 5, 4, 3, 2, 0]
        want = _compare(sim, (ids, off[:n_a + 1], n_a, ids, off[n_a:], n_b), a_idx, b_idx, 7, L, 0, ONLY_FIRST, segs, (L, "slices"))
        # ... and pair_ref itself against the documents cut out of the one CSR by hand
        for p in range(7):
            row, kept = ref.pair_row(docs[a_idx[p]], docs[n_a + b_idx[p]], L, 0, ONLY_FIRST, *map(list, segs))
            assert want[0][p, :len(row)].tolist() == [x for x, _, _ in row] and want[5][p].tolist() == list(kept)
        # a side with a filler in front of its ids (offsets that do not start at 0, an ids array of its own)
        b_ids2, b_off2 = ref.csr([len(d) for d in docs[n_a:]], rng, base=13)
        _compare(sim, (ids, off[:n_a + 1], n_a, b_ids2, b_off2, n_b), None, b_idx[:6], 6, L, KEEP_TAIL_B | PAD_LEFT, LONGEST_FIRST, segs,
                 (L, "base"))


def test_index_arithmetic_beyond_2_to_32(sim):
    """Rows of 2^31 + 1 entries, three pairs: flat indices pass 2^32.  No memory holds such an output: single groups of the kernel's mapping
    are evaluated where something happens -- the rows' starts and ends -- and compared with the row pair_ref.pair_row builds."""
    L, n_pairs = (1 << 31) + 1, 3
    rng = np.random.default_rng(20263)
    a_ids, a_off = ref.csr([5, 0, 9], rng)
    b_ids, b_off = ref.csr([2, 7, 1], rng)
    segs = ((0xA0000000,), (0xB0000000,), (0xC0000000, 0xC0000001))
    total = n_pairs * L
    assert total > (1 << 32) and total % 4 == 3
    for flags in (0, PAD_LEFT):
        e0 = sorted({e for p in range(n_pairs + 1) for e in range(max(0, (p * L - 24) // 4 * 4), min(total, p * L + 28), 4)})
        assert e0[-1] + 3 == total and sum(e > (1 << 32) for e in e0) > 10
        v, m, ty, sp, lens, kept, status = sim.groups(a_ids, a_off, 3, b_ids, b_off, 3, None, [2, 1, 0], n_pairs, L, flags, PAD_ID, e0,
                                                       LONGEST_FIRST, *segs)
        rows = []
        for p in range(n_pairs):
            a = a_ids[int(a_off[p]):int(a_off[p + 1])].tolist()
            b = b_ids[int(b_off[2 - p]):int(b_off[3 - p])].tolist()
            rows.append(ref.pair_row(a, b, L, flags, LONGEST_FIRST, *map(list, segs)))
        for g, e in enumerate(e0):
            for i in range(4):
                if e + i >= total:
                    assert v[g, i] == PAD_ID and (m[g, i], ty[g, i], sp[g, i]) == (0, 0, 0)       # (beyond the end: not stored by the kernel)
                    continue
                p, c = divmod(e + i, L)
                row = rows[p][0]
                j = c - (L - len(row) if flags & PAD_LEFT else 0)
                want = (row[j][0], 1, row[j][1], row[j][2]) if 0 <= j < len(row) else (PAD_ID, 0, 0, 1)
                assert (int(v[g, i]), m[g, i], ty[g, i], sp[g, i]) == want, (flags, e, i, p, c)
        assert lens.tolist() == [len(r[0]) for r in rows] and kept.tolist() == [list(r[1]) for r in rows] and status == 0


def test_grid_covers_every_span_once(sim):
    """the grid's x, then y and z: every span below 2^53 has exactly one workgroup, within the limits of a launch"""
    span = sim.geometry()["span"]
    X = (1 << 31) - 1
    for total in (0, 1, span, span + 1, 5 * span, X * span, X * span + 1, (1 << 41) + 5, 65535 * X * span, 65535 * X * span + 1, (1 << 57) + 123,
                  (1 << 63) - 1, 1 << 63):
        gx, gy, gz = sim.grid(total)
        spans = (total + span - 1) // span
        assert 1 <= gx <= X and 1 <= gy <= 65535 and 1 <= gz <= 65535, total
        assert gx * gy * gz >= spans and (gx * gy * gz - spans) < gx * gy + gx, total       # no span without a workgroup, less than a layer too many
        assert sim.span(0, 0, 0, gx, gy) == 0 and sim.span(gx - 1, gy - 1, gz - 1, gx, gy) == gx * gy * gz - 1
        if gy > 1:
            assert sim.span(gx - 1, 0, 0, gx, gy) + 1 == sim.span(0, 1, 0, gx, gy)
        if gz > 1:
            assert sim.span(gx - 1, gy - 1, 0, gx, gy) + 1 == sim.span(0, 0, 1, gx, gy)
        if spans <= X:
            assert (gx, gy, gz) == (max(spans, 1), 1, 1)


# ------------------------------------------------------------------------------------------ 4. pair_ref against hand-written examples
def test_ref_bert_form_by_hand():
    CLS, SEP, PAD = 101, 102, 0
    a_ids, a_off = np.array([11, 12, 13, 14, 15, 21], dtype=np.uint32), np.array([0, 5, 5, 6], dtype=np.uint64)      # [11..15], [], [21]
    b_ids, b_off = np.array([31, 32, 41, 42, 43, 44], dtype=np.uint32), np.array([0, 2, 2, 6], dtype=np.uint64)      # [31 32], [], [41..44]
    out = ref.pair_ref(a_ids, a_off, 3, b_ids, b_off, 3, None, None, 3, 8, 0, PAD, LONGEST_FIRST, [CLS], [SEP], [SEP])
    rows, mask, ttype, special, lens, kept, status = out
    # budget 5.  pair 0: 5 + 2 -> A loses two; pair 1: both empty; pair 2: 1 + 4 fits
    assert rows.tolist() == [[CLS, 11, 12, 13, SEP, 31, 32, SEP], [CLS, SEP, SEP, 0, 0, 0, 0, 0], [CLS, 21, SEP, 41, 42, 43, 44, SEP]]
    assert mask.tolist() == [[1] * 8, [1, 1, 1, 0, 0, 0, 0, 0], [1] * 8]
    assert ttype.tolist() == [[0, 0, 0, 0, 0, 1, 1, 1], [0, 0, 1, 0, 0, 0, 0, 0], [0, 0, 0, 1, 1, 1, 1, 1]]
    assert special.tolist() == [[1, 0, 0, 0, 1, 0, 0, 1], [1, 1, 1, 1, 1, 1, 1, 1], [1, 0, 1, 0, 0, 0, 0, 1]]
    assert lens.tolist() == [8, 3, 8] and kept.tolist() == [[3, 2], [0, 0], [1, 4]] and status == 0
    # the same pairs crosswise (A reversed), tails kept, padding on the left, only the second side cut
    out = ref.pair_ref(a_ids, a_off, 3, b_ids, b_off, 3, [2, 1, 0], None, 3, 7, PAD_LEFT | KEEP_TAIL_A | KEEP_TAIL_B, PAD, ONLY_SECOND,
                       [CLS], [SEP], [SEP])
    assert out[0].tolist() == [[0, CLS, 21, SEP, 31, 32, SEP], [0, 0, 0, 0, CLS, SEP, SEP], [CLS, 12, 13, 14, 15, SEP, SEP]]
    assert out[5].tolist() == [[1, 2], [0, 0], [4, 0]] and out[4].tolist() == [6, 3, 7]
    assert out[2].tolist() == [[0, 0, 0, 0, 1, 1, 1], [0, 0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 0, 1]]
    # an index that names no document: that side is empty, the status says so
    out = ref.pair_ref(a_ids, a_off, 3, b_ids, b_off, 3, [0, -1, 3], [2, 2, 0], 3, 12, 0, PAD, ONLY_FIRST, [CLS], [SEP], [SEP])
    assert out[0][1].tolist() == [CLS, SEP, 41, 42, 43, 44, SEP, 0, 0, 0, 0, 0] and out[0][2].tolist() == [CLS, SEP, 31, 32, SEP] + [0] * 7
    assert out[6] == 1 and out[5].tolist() == [[5, 4], [0, 4], [0, 2]]


def test_ref_roberta_form_and_the_tie_rule_by_hand():
    S, E, PAD = 0, 2, 1               # <s> a </s></s> b </s>
    a_ids, a_off = np.array([10, 11, 12, 13, 14, 15], dtype=np.uint32), np.array([0, 6], dtype=np.uint64)
    b_ids, b_off = np.array([20, 21, 22, 23, 24, 25], dtype=np.uint32), np.array([0, 6], dtype=np.uint64)
    out = ref.pair_ref(a_ids, a_off, 1, b_ids, b_off, 1, None, None, 1, 11, 0, PAD, LONGEST_FIRST, [S], [E, E], [E])
    # budget 7, both 6 long: ties take from B first, so A keeps ceil(7 / 2) = 4 and B 3
    assert out[0].tolist() == [[S, 10, 11, 12, 13, E, E, 20, 21, 22, E]]
    assert out[2].tolist() == [[0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1]] and out[3].tolist() == [[1, 0, 0, 0, 0, 1, 1, 0, 0, 0, 1]]
    assert out[5].tolist() == [[4, 3]]
    assert ref.truncate(6, 6, 7, LONGEST_FIRST) == (4, 3) and ref.truncate(6, 6, 6, LONGEST_FIRST) == (3, 3)
    assert ref.truncate(2, 9, 7, LONGEST_FIRST) == (2, 5) and ref.truncate(9, 2, 7, LONGEST_FIRST) == (5, 2)
    assert ref.truncate(9, 2, 7, ONLY_SECOND) == (7, 0) and ref.truncate(9, 2, 7, ONLY_FIRST) == (5, 2)
    assert ref.truncate(3, 9, 7, ONLY_FIRST) == (0, 7) and ref.truncate(3, 9, 7, ONLY_SECOND) == (3, 4)


# ------------------------------------------------------------------------------------------ 5. the Python surface refuses before it works
def test_check_pair_args():
    import torch
    from splintr_amd.device import check_pair_args
    check_pair_args(8, 0)
    check_pair_args(3, 0xFFFFFFFF, [1], (2,), [3], "only_second", "left", "left", "left", torch.int64)
    for kw, word in ((dict(dtype=torch.int16), "dtype"), (dict(truncation="shortest_first"), "truncation"),
                     (dict(truncation_side_a="middle"), "truncation_side_a"), (dict(truncation_side_b="up"), "truncation_side_b"),
                     (dict(padding_side="both"), "padding_side"), (dict(prefix=[1] * 33), "prefix"), (dict(middle="ab"), "middle"),
                     (dict(suffix=[1 << 32]), "suffix"), (dict(suffix=[-1]), "suffix"), (dict(prefix=[1.5]), "prefix")):
        with pytest.raises(ValueError, match=word):
            check_pair_args(8, 0, **kw)
    with pytest.raises(ValueError, match="pad_id"):
        check_pair_args(8, 1 << 32)
    with pytest.raises(ValueError, match="row length"):
        check_pair_args(0, 0)
    with pytest.raises(ValueError, match="row length"):
        check_pair_args(2, 0, [1], [2], [3])


def test_encode_batch_pairs_validates_before_anything_goes_to_the_device():
    """Bad arguments raise ValueError BEFORE the texts are packed, uploaded or encoded: a tokenizer object without a handle (and texts
    that could not even be packed) is enough to see it."""
    import torch
    from splintr_amd import Tokenizer
    t = Tokenizer.__new__(Tokenizer)
    bad = [b"not a str"]
    with pytest.raises(ValueError, match="dtype"):
        t.encode_batch_pairs(bad, bad, 8, pad_id=0, dtype=torch.float32)
    with pytest.raises(ValueError, match="truncation"):
        t.encode_batch_pairs(bad, bad, 8, pad_id=0, truncation="longest")
    with pytest.raises(ValueError, match="padding_side"):
        t.encode_batch_pairs(bad, bad, 8, pad_id=0, padding_side="up")
    with pytest.raises(ValueError, match="row length"):
        t.encode_batch_pairs(bad, bad, 2, pad_id=0, prefix=[1], middle=[2], suffix=[3])
    with pytest.raises(ValueError, match="equally long"):
        t.encode_batch_pairs(bad, bad + bad, 8, pad_id=0)
    with pytest.raises(ValueError, match="cross"):
        t.encode_batch_pairs(bad, bad, 8, pad_id=0, cross=True, a_index=[0])
    with pytest.raises(ValueError, match="texts_a"):
        t.encode_batch_pairs("one string", bad, 8, pad_id=0)
