"""spl_stream_decode_device without a GPU: the C ABI's refusals and the Python surface's ValueErrors through the real library, and the
mapping code the kernels run (splintr_amd/csrc/spl_k_stream.h, evaluated sequence by sequence and lane by lane by
tests/hostsim/stream_sim.cpp) against the two oracles of tests/stream_ref.py -- exhaustively over every string of up to four bytes of a
15-byte alphabet, fed one byte a step, whole, and at every two-way cut -- plus two mutants of the header that named checks must catch."""
import ctypes

import numpy as np
import pytest

import stream_ref as ref
from stream_ref import FINAL_ALL, REPLACE

I64, PAD_LEFT, SKIP_SPECIAL = 1, 2, 4
SPL_EINVAL = -1
GEOMETRIES = [(64, 64), (3, 2), (2, 5), (5, 3)]          # (slots of a window, bytes of a chunk); the first is the kernels'


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as entry
    entry.build()
    from splintr_amd import _ffi
    return _ffi


@pytest.fixture(scope="module")
def sim():
    import stream_sim
    stream_sim.lib()
    return stream_sim


@pytest.fixture(scope="module")
def tab():
    return ref.byte_table()


@pytest.fixture(scope="module")
def dtab(sim, tab):
    return sim.DeviceTable(tab, ref.MAX_ID)


# ------------------------------------------------------------------------------------------ 1. the C ABI and the Python surface
def test_symbols_flags_and_geometry(ffi, sim):
    import os
    import re
    from conftest import ROOT
    L = ffi.lib()
    for s in ("spl_stream_reserve_device", "spl_stream_decode_device"):
        assert hasattr(L, s) and s in ffi.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "splintr_hip.h")).read()
    for name, val in (("REPLACE", 1), ("FINAL_ALL", 2)):
        assert re.search(r"#define SPL_STREAM_%s\s+%du\b" % (name, val), hdr), name
        assert getattr(ffi, "SPL_STREAM_" + name) == val
    for cite in ("src/core/streaming.rs", "src/python/bindings.rs:591-640"):
        assert cite in hdr
    g = sim.geometry()
    assert g["wave"] == 64 and g["halo"] == 3 and g["seq_block"] <= 64 and g["lanes"] % 64 == 0 and g["one_lanes"] % 64 == 0
    assert sim.geometry("halo2")["halo"] == 2


def test_refusals_name_their_cause(ffi):
    """Every refusal comes before the handle or the device is touched: a dummy handle (never read) is enough, and none of the addresses
    below is ever dereferenced."""
    L = ffi.lib()
    handle = ctypes.create_string_buffer(64)
    h = ctypes.addressof(handle)
    A = 0x10000
    O = ffi.SplDecodeOpts

    def call(t=h, ids=A, ln=None, n=3, o=None, sf=0, fin=None, s_in=A, s_out=A, out=A, cap=64, oo=A):
        o = O(0, 1) if o is None else o
        return L.spl_stream_decode_device(t, ids, ln, n, ctypes.byref(o) if o is not False else None, sf, fin, s_in, s_out, out, cap, oo, None)

    def refused(rc, *words):
        msg = L.spl_last_error().decode()
        assert rc == SPL_EINVAL, (rc, msg)
        for w in ("spl_stream_decode_device",) + words:
            assert w in msg, (w, msg)

    refused(call(t=None), "null handle")
    refused(call(o=False), "options")
    refused(call(s_in=None), "d_state_in is null")
    refused(call(s_out=None), "d_state_out is null")
    refused(call(oo=None), "d_out_off is null")
    refused(call(ids=None), "d_ids is null")
    refused(call(out=None), "d_bytes is null", "bytes_capacity")
    short = O(0, 1)
    for size in (0, 8, 4097):
        short.struct_size = size
        refused(call(o=short), "struct_size")
    refused(call(o=O(8, 1)), "unknown flag bit 0x8")
    refused(call(sf=4), "unknown stream_flags bit 0x4")
    refused(call(sf=0x80000001), "unknown stream_flags bit 0x80000000")
    refused(call(o=O(0, 0)), "row_len is 0")
    refused(call(o=O(PAD_LEFT, 4)), "SPL_DECODE_PAD_LEFT")
    refused(call(out=A + 8), "d_bytes", "16-byte")
    refused(call(n=1 << 31), "n_seqs >= 2^31")
    # a LONGER struct is accepted and its tail ignored: the refusal that follows is about something else
    big = (ctypes.c_uint32 * 16)(64, 0, 0, 0xFFFFFFFF, 0xFFFFFFFF)
    refused(call(o=ctypes.cast(big, ctypes.POINTER(O)).contents), "row_len is 0")
    # the reserve call, and the option
    assert L.spl_stream_reserve_device(None, 10) == SPL_EINVAL and "null handle" in L.spl_last_error().decode()
    assert L.spl_stream_reserve_device(h, 1 << 31) == SPL_EINVAL and "2^31" in L.spl_last_error().decode()


def test_python_surface_validates_before_anything_goes_to_the_device():
    import torch
    from splintr_amd import Tokenizer
    from splintr_amd import device as dv
    t = Tokenizer.__new__(Tokenizer)
    ids = torch.zeros((4, 2), dtype=torch.int64)
    st = torch.zeros(4, dtype=torch.int64)
    chk = dv.check_stream_args
    with pytest.raises(ValueError, match="errors"):
        chk(ids, None, st, errors="strict")
    with pytest.raises(ValueError, match="max_bytes"):
        chk(ids, None, st, max_bytes=-1)
    with pytest.raises(ValueError, match="dtype"):
        chk(ids.to(torch.int16), None, st)
    with pytest.raises(ValueError, match="rank"):
        chk(ids.reshape(2, 2, 2), None, st)
    with pytest.raises(ValueError, match="contiguous"):
        chk(torch.zeros((2, 4), dtype=torch.int64).t(), None, st)
    with pytest.raises(ValueError, match="at least one id"):
        chk(torch.zeros((4, 0), dtype=torch.int64), None, st)
    with pytest.raises(ValueError, match="lengths"):
        chk(ids, torch.zeros(4, dtype=torch.int64), st)
    with pytest.raises(ValueError, match="state"):
        chk(ids, None, st.to(torch.int32))
    with pytest.raises(ValueError, match="state"):
        chk(ids, None, torch.zeros(5, dtype=torch.int64))
    with pytest.raises(ValueError, match="state_out"):
        chk(ids, None, st, state_out=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="final"):
        chk(ids, None, st, final=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="on a GPU"):
        chk(ids, torch.zeros(4, dtype=torch.int32), st, final=torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="on a GPU"):
        dv.stream_decode_device(t, ids[:, 0].contiguous(), None, st, max_bytes=16)
    with pytest.raises(ValueError, match="errors"):
        dv.DeviceStreamingDecoder(t, 4, errors="ignore")
    with pytest.raises(ValueError, match="batch_size"):
        dv.DeviceStreamingDecoder(t, -1)


# ------------------------------------------------------------------------------------------ 2. the oracles against examples by hand
def test_ref_by_hand(tab):
    h = ref.make(tab)
    assert h.step([0xE4]) == b"" and h.pending_bytes == 1 and not h.stalled
    assert h.step([0xBD, 0xA0, 0x41, 0xF0]) == "你A".encode() and h.pending_bytes == 1
    assert h.step([], final=True) == ref.FFFD and h.pending_bytes == 0
    assert h.step([0x41, 0x80, 0x42]) == b"A" and h.stalled and h.pending_bytes == 2
    assert h.step([0x43]) == b"" and h.pending_bytes == 3 and h.step([], final=True) == b"" and h.stalled
    r = ref.make(tab, replace=True)
    assert r.step([0x41, 0x80, 0x42, 0xF0, 0x90]) == b"A" + ref.FFFD + b"B" and r.pending_bytes == 2
    assert r.step([0x41]) == ref.FFFD + b"A" and r.pending_bytes == 0
    assert r.step([0xE0, 0x80]) == ref.FFFD * 2 and r.step([0xC2], final=True) == ref.FFFD
    assert [ref.st_count(0x2_00_A0E0 | 0), ref.st_pending(0x0200A0E0)] == [2, b"\xe0\xa0"]
    assert ref.st_well_formed(0x0200A0E0) and not ref.st_well_formed(0x0100A0E0) and ref.st_well_formed((7 << 32) | (1 << 26))
    assert not ref.st_well_formed((7 << 32) | (1 << 26) | 0x41) and ref.st_pending_bytes((7 << 32) | (1 << 26)) == 7


# ------------------------------------------------------------------------------------------ 3. the mapping code the kernels run
def _sflags(replace):
    return REPLACE if replace else 0


def _steps(sim, dtab, replace, lanes, chunk, mutant=""):
    """one byte per step (K = 1), four steps, then final"""
    strings = ref.alphabet_strings()
    rows, lens = ref.rows_of(strings)
    want = ref.alphabet_oracle(replace, "steps")
    state = np.zeros(len(strings), dtype=np.uint64)
    kw = dict(flags=0, sflags=_sflags(replace), capacity=3 * len(strings) + 16, lanes=lanes, chunk=chunk, mutant=mutant)
    for k in range(4):
        raw, off, state = sim.step(dtab, rows[:, k:k + 1], (lens > k).astype(np.int32), state, three=bool(k & 1), **kw)
        ref.check_step(("steps", replace, k), raw, off, state, want[k])
    kw["sflags"] |= FINAL_ALL
    raw, off, state = sim.step(dtab, rows[:, :1], np.zeros(len(strings), dtype=np.int32), state, three=True, **kw)
    ref.check_step(("steps", replace, "final"), raw, off, state, want[4])


def _whole(sim, dtab, replace, lanes, chunk, mutant=""):
    """all bytes in one call (K = 4), then final through d_final"""
    strings = ref.alphabet_strings()
    rows, lens = ref.rows_of(strings)
    want = ref.alphabet_oracle(replace, "whole")
    state = np.zeros(len(strings), dtype=np.uint64)
    kw = dict(flags=0, sflags=_sflags(replace), capacity=12 * len(strings) + 16, lanes=lanes, chunk=chunk, mutant=mutant)
    raw, off, state = sim.step(dtab, rows, lens, state, three=True, **kw)
    ref.check_step(("whole", replace), raw, off, state, want[0])
    raw, off, state = sim.step(dtab, rows, np.zeros(len(strings), dtype=np.int32), state, final=np.ones(len(strings), dtype=np.uint8), **kw)
    ref.check_step(("whole", replace, "final"), raw, off, state, want[1])


_cut_memo = {}


def _cut_cases():
    if not _cut_memo:
        strings = [s for s in ref.alphabet_strings() if len(s) >= 2]
        first, second = [], []
        for s in strings:
            for c in range(1, len(s)):
                first.append(s[:c])
                second.append(s[c:])
        _cut_memo["rows"] = (ref.rows_of(first), ref.rows_of(second))
        for replace in (False, True):
            bt = ref.Batch(ref.byte_table(), len(first), 0, replace)
            (r1, l1), (r2, l2) = _cut_memo["rows"]
            _cut_memo[replace] = [bt.step(r1, l1), bt.step(r2, l2, np.ones(len(first), dtype=np.uint8))]
    return _cut_memo


def _cuts(sim, dtab, replace, lanes, chunk, mutant=""):
    """every two-way cut of every string: the first part in one call, the second with final in the next"""
    cases = _cut_cases()
    (r1, l1), (r2, l2) = cases["rows"]
    assert len(l1) == 158850
    state = np.zeros(len(l1), dtype=np.uint64)
    kw = dict(flags=0, sflags=_sflags(replace), capacity=15 * len(l1) + 16, lanes=lanes, chunk=chunk, mutant=mutant)
    raw, off, state = sim.step(dtab, r1, l1, state, three=True, **kw)
    ref.check_step(("cut", replace, 1), raw, off, state, cases[replace][0])
    raw, off, state = sim.step(dtab, r2, l2, state, three=True, in_place=True, final=np.ones(len(l1), dtype=np.uint8), **kw)
    ref.check_step(("cut", replace, 2), raw, off, state, cases[replace][1])


@pytest.mark.parametrize("replace", [False, True], ids=["hold", "replace"])
def test_exhaustive_one_byte_per_step(sim, dtab, replace):
    for lanes, chunk in GEOMETRIES[:2]:
        _steps(sim, dtab, replace, lanes, chunk)


@pytest.mark.parametrize("replace", [False, True], ids=["hold", "replace"])
def test_exhaustive_whole_in_one_call(sim, dtab, replace):
    for lanes, chunk in GEOMETRIES:
        _whole(sim, dtab, replace, lanes, chunk)


@pytest.mark.parametrize("replace", [False, True], ids=["hold", "replace"])
def test_exhaustive_every_two_way_cut(sim, dtab, replace):
    for lanes, chunk in GEOMETRIES[:2]:
        _cuts(sim, dtab, replace, lanes, chunk)


def _straddle(sim, tab, dtab, replace, lanes, chunk, flags=0, mutant=""):
    rows, lens = ref.straddle_rows()
    r = rows if flags & I64 else rows.astype(np.uint32)
    bt = ref.Batch(tab, len(rows), flags, replace)
    state = np.zeros(len(rows), dtype=np.uint64)
    kw = dict(flags=flags, sflags=_sflags(replace), lanes=lanes, chunk=chunk, mutant=mutant)
    for step in range(2):                     # the second step starts from the two pending bytes of CH3 (or stalled)
        want = bt.step(rows, lens)
        need = sum(len(w) for w in want[0])
        raw, off, state = sim.step(dtab, r, lens, state, capacity=need, three=bool(step), **kw)
        assert int(off[-1]) == need
        ref.check_step(("straddle", replace, lanes, chunk, step), raw, off, state, want)


@pytest.mark.parametrize("replace", [False, True], ids=["hold", "replace"])
def test_long_tokens_straddle_every_chunk_edge(sim, tab, dtab, replace):
    for lanes, chunk in GEOMETRIES + [(64, 4), (7, 64), (1, 1)]:
        for flags in (0, I64, SKIP_SPECIAL):
            _straddle(sim, tab, dtab, replace, lanes, chunk, flags)


@pytest.mark.parametrize("replace", [False, True], ids=["hold", "replace"])
def test_zero_length_slots_and_idle_sequences(sim, tab, dtab, replace):
    """unknown ids, -1 / -100 / 2^32 + 0x41 as int64, skipped specials: they add nothing, wherever they stand; a row of nothing else, and
    len 0, leave a non-zero state bit for bit"""
    E, S, F = ref.CH3[0], ref.SPECIAL, ref.FAR
    prelude = np.full((5, 9), 0x41, dtype=np.int64)
    prelude[1:4, :2] = [E, ref.CH3[1]]
    prelude[4, 0] = 0x80
    pre_len = np.array([1, 2, 2, 2, 9], dtype=np.int32)
    rows = np.array([[E, -1, ref.CH3[1], -100, ref.CH3[2], (1 << 32) + 0x41, 311],
                     [-1, -100, 299, 257, 311, 1 << 32, -5],
                     [S, E, F, ref.CH3[1], S, S, 0x41],
                     [0x41, 0x42, 0x43, 0x44, 0x45, 0x46, 0x47],
                     [0x80, 0x41, 0x42, 0x43, 0x44, 0x45, 0x46]], dtype=np.int64)
    pend2 = (2 << 24) | (ref.CH3[1] << 8) | ref.CH3[0]
    for lanes, chunk in GEOMETRIES:
        for flags in (I64, I64 | SKIP_SPECIAL):
            kw = dict(flags=flags, sflags=_sflags(replace), capacity=96, lanes=lanes, chunk=chunk)
            bt = ref.Batch(tab, 5, flags, replace)
            raw, off, start = sim.step(dtab, prelude, pre_len, np.zeros(5, dtype=np.uint64), **kw)
            ref.check_step(("prelude", lanes, chunk, flags), raw, off, start, bt.step(prelude, pre_len))
            assert start.tolist() == [0, pend2, pend2, pend2, 0 if replace else (9 << 32) | (1 << 26)]
            raw, off, st = sim.step(dtab, rows, None, start, **kw)
            ref.check_step(("zero-length", lanes, chunk, flags), raw, off, st, bt.step(rows))
            assert raw[:3] == ref.CH3 and int(off[1]) == int(off[2]) == 3                     # row 0: the character; row 1: nothing
            assert int(st[0]) == 0 and int(st[1]) == pend2, [hex(int(x)) for x in st]         # ... and its state bit for bit
            if not replace:
                assert [ref.st_held(x) for x in st[2:]] == [5 if flags & SKIP_SPECIAL else 25, 9, 16]
            # len 0 (and a negative one): every state as it was, bit for bit, three-launch and one-launch form, in place and not
            for three in (False, True):
                for in_place in (False, True):
                    raw, off, st2 = sim.step(dtab, rows, np.array([0, -3, 0, 0, 0], dtype=np.int32), start, three=three, in_place=in_place, **kw)
                    assert raw == b"" and off.tolist() == [0] * 6 and st2.tolist() == start.tolist()


def test_every_capacity_and_no_sequence(sim, tab, dtab):
    rows, lens = ref.straddle_rows()
    rows, lens = rows[:4], lens[:4]
    for replace in (False, True):
        bt = ref.Batch(tab, len(rows), I64, replace)
        want = bt.step(rows, lens)
        whole = b"".join(want[0])
        full = None
        for cap in list(range(0, 40)) + [len(whole) - 1, len(whole), len(whole) + 1]:
            raw, off, st = sim.step(dtab, rows, lens, np.zeros(4, dtype=np.uint64), flags=I64, sflags=_sflags(replace), capacity=cap,
                                    lanes=5, chunk=3, three=bool(cap & 1))
            assert raw == whole[:cap] and int(off[-1]) == len(whole), (replace, cap)
            full = st if full is None else full
            assert st.tolist() == full.tolist()                          # the state after a short call is the state after a full one
        raw, off, st = sim.step(dtab, rows[:0], None, np.zeros(0, dtype=np.uint64), flags=I64, sflags=_sflags(replace), capacity=16)
        assert raw == b"" and off.tolist() == [0]


# ------------------------------------------------------------------------------------------ 4. mutants the checks above must catch
def test_mutant_second_byte_not_narrowed_is_caught(sim, tab):
    """a continuation check that ignores the narrowed second byte after E0 / ED / F0 / F4: the exhaustive checks fail in both modes"""
    sim.lib("wide_second")
    dt = sim.DeviceTable(tab, ref.MAX_ID)
    for replace in (False, True):
        with pytest.raises(AssertionError):
            _whole(sim, dt, replace, 64, 64, mutant="wide_second")
        with pytest.raises(AssertionError):
            _steps(sim, dt, replace, 64, 64, mutant="wide_second")
        with pytest.raises(AssertionError):
            _cuts(sim, dt, replace, 64, 64, mutant="wide_second")


def test_mutant_halo_of_two_bytes_is_caught(sim, tab):
    """a halo of 2 bytes: a four-byte character's lead does not see its last byte -- the exhaustive whole-string check and the straddle
    check fail in both modes"""
    sim.lib("halo2")
    dt = sim.DeviceTable(tab, ref.MAX_ID)
    for replace in (False, True):
        with pytest.raises(AssertionError):
            _whole(sim, dt, replace, 64, 64, mutant="halo2")
        with pytest.raises(AssertionError):
            _straddle(sim, tab, dt, replace, 64, 64, mutant="halo2")
