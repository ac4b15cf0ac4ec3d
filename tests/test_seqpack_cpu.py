"""spl_seqpack_device without a GPU: tests/seqpack_ref.py against the examples written out by hand, the decisions the kernels run
(splintr_amd/csrc/spl_k_seqpack.h, evaluated for every output element by tests/hostsim/seqpack_sim.cpp, which also restates the plan
kernels' phases lane by lane) against that reference, and the C ABI's symbols, struct layout and refusals."""
import ctypes
import os
import re

import numpy as np
import pytest

import seqpack_ref as ref
from conftest import ROOT

SPL_EINVAL = -1
STRATEGIES = ("next_fit", "best_fit_decreasing")


@pytest.fixture(scope="module")
def sim():
    import seqpack_sim
    seqpack_sim.lib()
    return seqpack_sim


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as entry
    entry.build()
    from splintr_amd import _ffi
    return _ffi


# ------------------------------------------------------------------------------------------ 1. the reference
@pytest.mark.parametrize("L, lengths, strategy, rows", [
    (10, [6, 5, 5, 4], "next_fit", [[0], [1, 2], [3]]),
    (10, [6, 5, 5, 4], "best_fit_decreasing", [[0, 3], [1, 2]]),
    (10, [3, 0, 7, 1, 12, 10, 5, 5], "next_fit", [[0, 2], [3], [4], [5], [6, 7]]),
    (10, [3, 0, 7, 1, 12, 10, 5, 5], "best_fit_decreasing", [[4], [5], [2, 0], [6, 7], [3]]),
    (7, [4, 4, 3, 3, 3, 3], "best_fit_decreasing", [[0, 3], [1, 2], [4, 5]]),
])
def test_reference_examples(L, lengths, strategy, rows):
    p = ref.plan(lengths, L, strategy)
    assert p.rows == rows
    if 0 in lengths:
        assert tuple(p.place[lengths.index(0)]) == (-1, -1)
    if 12 in lengths:
        assert p.clen[4] == 10 and p.cut[4] and sum(p.cut) == 1
    for r, row in enumerate(rows):                       # no gaps, in placement order
        c = 0
        for i in row:
            assert tuple(p.place[i]) == (r, c)
            c += p.clen[i]


def test_reference_outputs_by_hand():
    out = ref.pack([[11, 12, 13], [], [21, 22]], 4, "next_fit", pad_id=9, labels=[[11, -100, 13], [], [21, 22]], byte_arrays=([[1, 1, 1], [], [2, 2]],) + (None,) * 3,
                   fills=(7, 0, 0, 0))
    assert out.input_ids.tolist() == [[11, 12, 13, 9], [21, 22, 9, 9], [9, 9, 9, 9]]
    assert out.labels.tolist() == [[-100, -100, 13, -100], [-100, 22, -100, -100], [-100] * 4]        # (MASK_FIRST)
    assert out.bytes[0].tolist() == [[1, 1, 1, 7], [2, 2, 7, 7], [7, 7, 7, 7]]
    assert out.position_ids.tolist() == [[0, 1, 2, 0], [0, 1, 0, 0], [0] * 4] and out.seq_ids.tolist() == [[0, 0, 0, -1], [2, 2, -1, -1], [-1] * 4]
    assert out.seq_place.tolist() == [[0, 0], [-1, -1], [1, 0]] and out.row_fill.tolist() == [3, 2, 0]
    assert out.cu_seqlens[:5].tolist() == [0, 3, 4, 6, 8] and out.n.tolist() == [2, 5, 5, 0]


# ------------------------------------------------------------------------------------------ 2. the kernels' decisions against the reference
def _check(sim, lengths, L, strategy, *, form="rows", i64=False, pad_left=False, keep_tail=False, mask_first=True, max_rows=None, lds_max=None,
           null=(), companions=True):
    seqs, labels, byts = sim.content(lengths)
    inp = sim.Inputs(seqs, form, i64=i64, pad_left=pad_left, labels=labels if companions else None,
                     byte_arrays=byts if companions else (None,) * 4)
    kw = dict(max_rows=max_rows, pad_id=77, ignore_index=-100, fills=(1, 2, 3, 255), keep_tail=keep_tail, mask_first=mask_first)
    got = sim.run(inp, L, strategy, lds_max=lds_max, null=null, **kw)
    want = ref.pack(seqs, L, strategy, labels=labels if companions else None, byte_arrays=byts if companions else (None,) * 4, **kw)
    sim.assert_equal(got, want)
    if not null:
        ref.check_invariants(got, lengths, L, len(lengths) if max_rows is None else max_rows)
    return got


def _variant(k):
    """the k-th combination of input form, dtype, padding side of the input and kept end"""
    return dict(form=("rows", "csr")[k & 1], i64=bool(k & 2), pad_left=bool(k & 4), keep_tail=bool(k & 8))


def test_grid_against_reference(sim):
    """every row_len x n_seqs of the grid, both strategies, the sixteen input variants taken in turn; best_fit_decreasing never needs
    more rows than next_fit ON THESE INPUTS (a property of what is tested, not a theorem)."""
    for k, (name, lengths, L) in enumerate(sim.grid_cases()):
        rows = {}
        for s, strategy in enumerate(STRATEGIES):
            rows[strategy] = int(_check(sim, lengths, L, strategy, **_variant(k + 5 * s)).n[0])
        assert rows["best_fit_decreasing"] <= rows["next_fit"], name


def test_every_input_variant(sim):
    lengths = [5, 0, 9, 3, 12, 7, 7, 1, 0, 8, 2, 11] * 6
    for k in range(16):
        for strategy in STRATEGIES:
            for mask_first in (True, False):
                _check(sim, lengths, 9, strategy, mask_first=mask_first, **_variant(k))


def test_shaped_lengths(sim):
    for k, (name, lengths, L) in enumerate(sim.shaped_cases()):
        rows = {s: int(_check(sim, lengths, L, s, **_variant(k)).n[0]) for s in STRATEGIES}
        assert rows["best_fit_decreasing"] <= rows["next_fit"], name
    got = _check(sim, [3, 7, 4, 6, 5, 5, 10, 1, 9], 10, "next_fit")
    assert got.row_fill[:5].tolist() == [10, 10, 10, 10, 10] and int(got.n[0]) == 5         # fills that end exactly at row_len
    got = _check(sim, [4, 4, 3, 3, 3, 3], 7, "best_fit_decreasing")
    assert got.seq_place.tolist() == [[0, 0], [1, 0], [1, 4], [0, 4], [2, 0], [2, 3]]           # the LIFO tie


def test_launch_shape_thresholds(sim):
    """n_seqs one below, at and one above every threshold: the LDS / work-buffer switch of both plans (lowered by the option, and at its
    default), the plan workgroup's stride, and best_fit_decreasing's pool bound L + 1 + 2 n <= pool words"""
    g = sim.geometry()
    rng = np.random.default_rng(3)
    for lds_max in (0, 64):
        for n in (63, 64, 65):
            for strategy in STRATEGIES:
                _check(sim, rng.integers(0, 9, size=n).tolist(), 7, strategy, lds_max=lds_max)
    for n in (g["plan_lanes"] - 1, g["plan_lanes"], g["plan_lanes"] + 1, g["lds_max"] - 1, g["lds_max"], g["lds_max"] + 1):
        for strategy in STRATEGIES:
            _check(sim, rng.integers(0, 19, size=n).tolist(), 16, strategy, form="csr", companions=False)
    L = g["bfd_max_l"]
    half = (g["pool"] - L - 1) // 2
    for n in (half - 1, half, half + 1):
        lengths = rng.integers(1, 64, size=n).tolist()
        lengths[0], lengths[5], lengths[n // 2] = L, L - 3, L // 2
        seqs = [[i + 1] * l for i, l in enumerate(lengths)]
        got = sim.run(sim.Inputs(seqs, "csr"), L, "best_fit_decreasing", null=("labels", "b0", "b1", "b2", "b3", "mask", "pos", "sid"), max_rows=1)
        p = ref.plan(lengths, L, "best_fit_decreasing")
        assert (got.seq_place == p.place).all() and int(got.n[0]) == len(p.rows)


def test_max_rows_below_the_need(sim):
    lengths = [5, 6, 7, 3, 9, 2, 8, 4, 1, 9, 9]
    for strategy in STRATEGIES:
        need = len(ref.plan(lengths, 9, strategy).rows)
        for R in (0, 1, need - 1, need, need + 1):
            got = _check(sim, lengths, 9, strategy, max_rows=R)          # (run() checks the canary behind row max_rows of every array)
            assert int(got.n[0]) == need


def test_optional_outputs(sim):
    lengths = [5, 0, 9, 3, 12, 7, 7, 1]
    for strategy in STRATEGIES:
        for name in sim.OUT_NAMES:
            _check(sim, lengths, 9, strategy, null=(name,))
        _check(sim, lengths, 9, strategy, null=sim.OUT_NAMES)
        _check(sim, lengths, 9, strategy, companions=False)


def test_bad_input_is_reported_and_empty(sim):
    seqs, labels, byts = sim.content([4, 3, 5, 2, 6])
    for strategy in STRATEGIES:
        for over in ([4, -1, 5, 2, 6], [4, 3, 7, 2, 6], [4, 3, 5, -2147483648, 6]):
            bad = [i for i, (a, b) in enumerate(zip(over, [4, 3, 5, 2, 6])) if a != b]
            inp = sim.Inputs(seqs, "rows", L_in=6, labels=labels, lengths_override=over)
            got = sim.run(inp, 8, strategy)
            sim.assert_equal(got, ref.pack(seqs, 8, strategy, labels=labels, bad=bad))
            assert got.status == 1
        off = [3, 7, 6, 11, 13, 19]                      # offsets that decrease: sequence 1 is [7, 6)
        inp = sim.Inputs(seqs, "csr", off_override=off)
        got = sim.run(inp, 8, strategy)
        seqs2 = [inp.ids[off[i]:off[i + 1]].tolist() if off[i + 1] >= off[i] else [] for i in range(5)]
        sim.assert_equal(got, ref.pack(seqs2, 8, strategy, bad=[1]))


def test_random_sweep(sim):
    rng = np.random.default_rng(11)
    for k in range(150):
        L = int(rng.integers(1, 40))
        n = int(rng.integers(0, 90))
        hi = int(rng.choice([2, L // 2 + 2, L + 3]))
        lengths = rng.integers(0, hi, size=n).tolist()
        rows = {s: int(_check(sim, lengths, L, s, **_variant(k)).n[0]) for s in STRATEGIES}
        assert rows["best_fit_decreasing"] <= rows["next_fit"]


def test_work_bytes(sim):
    prev = 0
    for n, R in ((0, 0), (0, 1), (1, 1), (63, 63), (64, 63), (64, 70), (4097, 4097)):
        b = sim.work_bytes(n, R)
        assert b % 16 == 0 and b >= prev
        prev = b


# ------------------------------------------------------------------------------------------ 3. the C ABI
def test_symbols_and_struct_layout(ffi):
    L = ffi.lib()
    for s in ("spl_seqpack_device", "spl_seqpack_work_bytes"):
        assert hasattr(L, s) and s in ffi.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "splintr_hip.h")).read()
    for name, val in (("NEXT_FIT", 0), ("BEST_FIT_DECREASING", 1), ("MASK_FIRST", 32), ("BFD_MAX_ROW_LEN", 32768)):
        assert re.search(r"#define SPL_SEQPACK_%s\s+%du\b" % (name, val), hdr), name
        assert getattr(ffi, "SPL_SEQPACK_" + name) == val
    assert ctypes.sizeof(ffi.SplSeqpackOpts) == 28 and ctypes.sizeof(ffi.SplSeqpackIn) == 80 and ctypes.sizeof(ffi.SplSeqpackOut) == 128
    for struct, cls in (("spl_seqpack_opts", ffi.SplSeqpackOpts), ("spl_seqpack_in", ffi.SplSeqpackIn), ("spl_seqpack_out", ffi.SplSeqpackOut)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [re.sub(r"\[.*", "", n.strip().split()[-1].lstrip("*")) for decl in body.split(";") if decl.strip() for n in decl.split(",")]
        assert fields == [f[0] for f in cls._fields_], struct
    assert L.spl_seqpack_work_bytes(100, 50, 0) == L.spl_seqpack_work_bytes(100, 50, 1) and L.spl_seqpack_work_bytes(100, 50, 0) % 16 == 0


def test_work_bytes_agree(ffi, sim):
    for n, R in ((0, 0), (1, 1), (65, 7), (4097, 4097)):
        assert ffi.lib().spl_seqpack_work_bytes(n, R, 0) == sim.work_bytes(n, R)


def test_refusals_name_their_cause(ffi):
    """Every refusal comes before the handle or the device is touched: a dummy handle (never read) is enough, and none of the addresses
    below is ever dereferenced."""
    L = ffi.lib()
    handle = ctypes.create_string_buffer(64)
    h = ctypes.addressof(handle)
    A = 0x10000
    In, O, Out = ffi.SplSeqpackIn, ffi.SplSeqpackOpts, ffi.SplSeqpackOut

    def call(t=h, i=None, o=None, out=None, work=A, **kw):
        i = In(3, 8, ids=A, lengths=A) if i is None else i
        o = O(0, 0, 8) if o is None else o
        out = Out(3, rows=A, status=A, **kw) if out is None else out
        ref_ = lambda x: None if x is False else ctypes.byref(x)
        return L.spl_seqpack_device(t, ref_(i), ref_(o), ref_(out), work, None)

    def refused(rc, *words):
        msg = L.spl_last_error().decode()
        assert rc == SPL_EINVAL, (rc, msg)
        for w in ("spl_seqpack_device",) + words:
            assert w in msg, (w, msg)

    refused(call(t=None), "null handle")
    refused(call(i=False), "input struct")
    refused(call(o=False), "options")
    refused(call(out=False), "output struct")
    refused(call(out=Out(3, status=A)), "d_rows is null")
    refused(call(out=Out(3, rows=A)), "d_status is null")
    refused(call(work=None), "d_work is null")
    for make in (lambda: In(3, 8, ids=A, lengths=A), lambda: O(0, 0, 8), lambda: Out(3, rows=A, status=A)):
        for size in (0, ctypes.sizeof(make()) - 4, 4097):
            s = make()
            s.struct_size = size
            refused(call(**{("i" if isinstance(s, In) else "o" if isinstance(s, O) else "out"): s}), "struct_size")
    refused(call(i=In(3, 8, ids=A, lengths=A, off=A)), "both input forms")
    refused(call(i=In(3, 8, ids=A)), "neither input form")
    refused(call(i=In(3, 8, lengths=A)), "d_ids is null")
    refused(call(i=In(3, 0, ids=A, lengths=A)), "in_len is 0")
    refused(call(o=O(128, 0, 8)), "unknown flag bit 0x80")
    for bit in (8, 16):
        refused(call(o=O(bit, 0, 8)), "SPL_COLLATE_BOS")
    refused(call(i=In(3, 0, ids=A, off=A), o=O(2, 0, 8)), "SPL_COLLATE_PAD_LEFT", "CSR")
    refused(call(o=O(0, 2, 8)), "unknown strategy")
    refused(call(o=O(0, 0, 0)), "row_len is 0")
    refused(call(o=O(0, 1, 32769)), "best_fit_decreasing", "32768")
    refused(call(i=In(1 << 31, 8, ids=A, lengths=A)), "n_seqs >= 2^31")
    refused(call(out=Out(1 << 31, rows=A, status=A)), "max_rows >= 2^31")
    refused(call(o=O(0, 0, 1 << 16), out=Out(1 << 15, rows=A, status=A, cu=A)), "d_cu", "2^31")
    for name in ("rows", "labels", "pos", "seq", "place", "fill", "cu", "n"):
        refused(call(out=Out(3, **{**dict(rows=A, status=A), name: A + 8})), "d_" + name, "16-byte")
    refused(call(work=A + 8), "d_work", "16-byte")
    refused(call(out=Out(3, rows=A, status=A, mask=A + 2)), "d_mask", "4-byte")
    refused(call(out=Out(3, rows=A, status=A, byte_arrays=(None, A + 1, None, None))), "byte output", "4-byte")
    refused(call(i=In(3, 8, ids=A, lengths=A + 2)), "d_lengths", "4-byte")
    refused(call(i=In(3, 0, ids=A, off=A + 4)), "d_off", "8-byte")


def test_python_surface_refuses_before_the_device():
    """ValueError for what the Python layer can see by itself -- no GPU, no tensors on a device."""
    torch = pytest.importorskip("torch")
    from splintr_amd import device as dv
    ok = dict(pad_id=0)
    dv.check_seqpack_args(8, **ok)
    for kw in (dict(strategy="first_fit"), dict(dtype=torch.int16), dict(pad_id=-1), dict(pad_id=1 << 32), dict(ignore_index=1 << 40),
               dict(truncation_side="up"), dict(padding_side="up"), dict(fills=(0, 0, 0)), dict(fills=(0, 0, 0, 256)), dict(max_rows=-1)):
        with pytest.raises(ValueError):
            dv.check_seqpack_args(8, **{**ok, **kw})
    for row_len in (0, -1, 1 << 32, True):
        with pytest.raises(ValueError):
            dv.check_seqpack_args(row_len, **ok)
    with pytest.raises(ValueError):
        dv.check_seqpack_args(32769, strategy="best_fit_decreasing", **ok)
    dv.check_seqpack_args(32769, strategy="next_fit", **ok)
