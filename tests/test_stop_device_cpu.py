"""spl_stop_match_device without a GPU: the C ABI's refusals and the Python surface's ValueErrors through the real library, and the mapping
code the kernels run (splintr_amd/csrc/spl_k_stop.h, evaluated sequence by sequence and lane by lane by tests/hostsim/stop_sim.cpp)
against the whole-text oracle of tests/stop_ref.py -- exhaustively over every text of up to eight bytes of {a, b, c} and a dozen stop
sets, fed whole, one byte a step and at every two-way cut -- plus two mutants of the header that named checks must catch."""
import ctypes
import itertools

import numpy as np
import pytest

import stop_ref as ref

SPL_EINVAL = -1
GEOMETRIES = [(64, 64), (3, 2), (5, 3), (1, 1)]          # (lanes of a wavefront, end positions of a chunk); the first is the kernels'
STOP_SETS = [
    [b"a"], [b"ab", b"b"], [b"abc", b"bc"], [b"ab", b"abc"], [b"aa"], [b"abca", b"bcab"], [b"bc", b"abc", b"bc"], [b"c", b"cc", b"ccc"],
    [b"abab"], [b"ba", b"ab", b"cab"], [b"aaaa", b"aab"], [b"cb", b"bcb", b"abcb", b"b"],
]


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as entry
    entry.build()
    from splintr_amd import _ffi
    return _ffi


@pytest.fixture(scope="module")
def sim():
    import stop_sim
    stop_sim.lib()
    return stop_sim


def drive(sim, tab, feeds, *, masks=None, include=False, final_all=False, geometry=(64, 64), three=False, mutant="", in_place=False,
          capacity=None, check_rows=True):
    """feeds: per sequence a list of (data, final) -- one entry per call, the same number for every sequence.  Every call goes through the
    sim and is compared with the oracle: bytes, offsets, hits and (check_rows) the state rows bit for bit.  Returns per sequence (the
    concatenated output, the hit) and the released length after every call."""
    B = len(feeds)
    n_calls = len(feeds[0]) if B else 0
    seqs = [ref.Seq(ref.live_stops(tab, None if masks is None else masks[b]), include) for b in range(B)]
    state = np.zeros((B, ref.WORDS), dtype=np.uint64)
    outs, rel = [b""] * B, []
    msk = None if masks is None else np.array(masks, dtype=np.uint64)
    flags = (ref.INCLUDE if include else 0) | (ref.FINAL_ALL if final_all else 0)
    for c in range(n_calls):
        call = [feeds[b][c] for b in range(B)]
        data, off = ref.csr([d for d, _ in call])
        fin = None if final_all or not any(f for _, f in call) else np.array([1 if f else 0 for _, f in call], dtype=np.uint8)
        cap = int(off[-1]) + 64 * B if capacity is None else capacity
        got = sim.step(data, off, state, tab, mask=msk, final=fin, flags=flags, capacity=cap, lanes=geometry[0], chunk=geometry[1],
                       three=three, in_place=in_place, mutant=mutant)
        want = ref.run_calls(seqs, [[(d, f or final_all) for d, f in call]])[0]
        assert (got[1] == want[1]).all(), ("offsets", c)
        assert got[0] == want[0][:cap], ("bytes", c)
        assert (got[2] == want[2]).all(), ("hits", c)
        if check_rows:
            bad = np.nonzero((got[3] != want[3]).any(axis=1))[0]
            assert bad.size == 0, ("rows", c, bad[:4], got[3][bad[:1]], want[3][bad[:1]])
        if capacity is None:
            o = got[1].astype(np.int64)
            outs = [outs[b] + got[0][o[b]:o[b + 1]] for b in range(B)]
        state = got[3]
        rel.append(state[:, 1].astype(np.int64).copy())
    return outs, [q.hit for q in seqs], rel


def all_texts(alphabet, n):
    return [b"".join(t) for k in range(n + 1) for t in itertools.product(alphabet, repeat=k)]


# ------------------------------------------------------------------------------------------ 1. the C ABI and the Python surface
def test_symbols_flags_and_geometry(ffi, sim):
    import os
    import re
    from conftest import ROOT
    L = ffi.lib()
    for s in ("spl_stop_reserve_device", "spl_stop_match_device", "spl_get_option"):
        assert hasattr(L, s) and s in ffi.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "splintr_hip.h")).read()
    for name, val in (("INCLUDE", "1u"), ("FINAL_ALL", "2u"), ("SLOTS", "64"), ("MAX_LEN", "64"), ("STATE_WORDS", "10")):
        assert re.search(r"#define SPL_STOP_%s\s+%s\b" % (name, val), hdr), name
        assert getattr(ffi, "SPL_STOP_" + name) == int(val.rstrip("u"))
    assert ffi.SPL_STOP_TABLE_BYTES == 4160 == ref.TABLE_BYTES
    assert "NO LIVE SEQUENCE'S MASK NAMES IT" in hdr and "profiles/stop_match.txt" in hdr
    g = sim.geometry()
    assert g["wave"] == 64 and g["halo"] == 63 and g["seq_block"] <= 64 and g["lanes"] % 64 == 0 and g["one_lanes"] % 64 == 0
    assert g["one_max"] <= g["one_cap"] == 1024 and g["table_bytes"] == 4160
    assert sim.geometry("halo62")["halo"] == 62


def test_refusals_name_their_cause(ffi):
    """Every refusal comes before the handle or the device is touched: a dummy handle (never read) is enough, and none of the addresses
    below is ever dereferenced."""
    L = ffi.lib()
    handle = ctypes.create_string_buffer(64)
    h = ctypes.addressof(handle)
    A = 0x10000

    def call(t=h, inb=A, icap=64, ioff=A, n=3, tab=A, mask=None, fin=None, fl=0, s_in=A, s_out=A, out=A, cap=64, oo=A, hit=A):
        return L.spl_stop_match_device(t, inb, icap, ioff, n, tab, mask, fin, fl, s_in, s_out, out, cap, oo, hit, None)

    def refused(rc, *words):
        msg = L.spl_last_error().decode()
        assert rc == SPL_EINVAL, (rc, msg)
        for w in ("spl_stop_match_device",) + words:
            assert w in msg, (w, msg)

    refused(call(t=None), "null handle")
    refused(call(tab=None), "d_table is null")
    refused(call(s_in=None), "d_state_in is null")
    refused(call(s_out=None), "d_state_out is null")
    refused(call(oo=None), "d_out_off is null")
    refused(call(hit=None), "d_hit is null")
    refused(call(ioff=None), "d_in_off is null")
    refused(call(inb=None), "d_in_bytes is null", "in_capacity")
    refused(call(out=None), "d_out_bytes is null", "out_capacity")
    refused(call(out=A + 8), "d_out_bytes", "16-byte")
    refused(call(fl=4), "unknown stop_flags bit 0x4")
    refused(call(fl=0x80000001), "unknown stop_flags bit 0x80000000")
    refused(call(n=1 << 31), "n_seqs >= 2^31")
    assert L.spl_stop_reserve_device(None, 10) == SPL_EINVAL and "null handle" in L.spl_last_error().decode()
    assert L.spl_stop_reserve_device(h, 1 << 31) == SPL_EINVAL and "2^31" in L.spl_last_error().decode()
    v = ctypes.c_int64(-7)
    assert L.spl_get_option(None, b"stop_one_max", ctypes.byref(v)) == SPL_EINVAL and v.value == -7
    assert L.spl_get_option(h, None, ctypes.byref(v)) == SPL_EINVAL and L.spl_get_option(h, b"stop_one_max", None) == SPL_EINVAL


def test_python_surface_validates_before_anything_goes_to_the_device():
    import torch
    from splintr_amd import device as dv
    for bad, word in (([""], "1 .. 64"), (["x" * 65], "1 .. 64"), (["a"] * 65, "at most 64"), ("ab", "list"), ([3], "str or bytes"),
                      (["é" * 33], "1 .. 64")):
        with pytest.raises(ValueError, match=word):
            dv.stop_table(bad)
    t = dv._stop_table_host(["ab", b"\xff", "é" * 32])
    assert t.shape == (4160,) and (t == ref.table([b"ab", b"\xff", "é" * 32])).all()
    inb, off = torch.zeros(32, dtype=torch.uint8), torch.zeros(5, dtype=torch.int64)
    st, tab = torch.zeros((4, 10), dtype=torch.int64), torch.from_numpy(t)
    chk = dv.check_stop_args
    with pytest.raises(ValueError, match="max_bytes"):
        chk(inb, off, st, tab, max_bytes=-1)
    with pytest.raises(ValueError, match="in_bytes"):
        chk(inb.to(torch.int8), off, st, tab)
    with pytest.raises(ValueError, match="in_off"):
        chk(inb, off.to(torch.int32), st, tab)
    with pytest.raises(ValueError, match="table"):
        chk(inb, off, st, tab[:100])
    with pytest.raises(ValueError, match="state must"):
        chk(inb, off, torch.zeros((4, 9), dtype=torch.int64), tab)
    with pytest.raises(ValueError, match="state_out"):
        chk(inb, off, st, tab, state_out=torch.zeros((3, 10), dtype=torch.int64))
    with pytest.raises(ValueError, match="mask"):
        chk(inb, off, st, tab, mask=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="final"):
        chk(inb, off, st, tab, final=torch.zeros(3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="GPU"):
        chk(inb, off, st, tab)
    with pytest.raises(ValueError, match="1 .. 64"):
        dv.DeviceStreamingDecoder(None, 4, stop=[""])


# ------------------------------------------------------------------------------------------ 2. exhaustive, against the whole-text oracle
@pytest.fixture(scope="module")
def texts8():
    return all_texts([b"a", b"b", b"c"], 8)


@pytest.mark.parametrize("k", range(len(STOP_SETS)))
def test_exhaustive_whole_and_byte_a_step(sim, texts8, k):
    """every text of up to 8 bytes over {a, b, c}: fed whole (both forms) and one byte a step -- output per step, hit and row bit for bit;
    property (iii): the same text and hit however the steps cut it; property (i): the released length never decreases"""
    tab = ref.table(STOP_SETS[k])
    whole, hit_w, _ = drive(sim, tab, [[(t, False)] for t in texts8])
    whole3, hit_3, _ = drive(sim, tab, [[(t, False)] for t in texts8], three=True, geometry=(3, 2))
    steps = [[(t[i:i + 1], False) for i in range(8)] for t in texts8]
    bytewise, hit_b, rel = drive(sim, tab, steps, geometry=(5, 3), three=(k % 2 == 1))
    assert whole == whole3 == bytewise and hit_w == hit_3 == hit_b
    for a, b in zip(rel, rel[1:]):
        assert (b >= a).all()
    # against the definition, spelled out once more for the whole text
    stops = ref.live_stops(tab)
    for t, o, h in zip(texts8, whole, hit_w):
        f = ref.first_hit(t, stops)
        assert (o, h) == ((t[:f[1]], f[2]) if f else (t[:len(t) - ref.held(t, stops)], -1))


@pytest.mark.parametrize("k", range(len(STOP_SETS)))
def test_exhaustive_every_two_way_cut(sim, texts8, k):
    """... and at every two-way cut; property (ii): what the first call released is a prefix of what the whole text releases"""
    tab = ref.table(STOP_SETS[k])
    stops = ref.live_stops(tab)
    pairs = [(t, c) for t in texts8 for c in range(1, len(t))]
    outs, hits, rel = drive(sim, tab, [[(t[:c], False), (t[c:], False)] for t, c in pairs], geometry=GEOMETRIES[k % 4], three=(k % 3 == 0))
    for (t, c), o, h in zip(pairs, outs, hits):
        f = ref.first_hit(t, stops)
        assert (o, h) == ((t[:f[1]], f[2]) if f else (t[:len(t) - ref.held(t, stops)], -1)), (t, c)
    for b, ((t, c), o) in enumerate(zip(pairs, outs)):                   # (ii) on the code's own `released` after the first call
        assert rel[0][b] <= len(o) == rel[1][b], (t, c)


def test_released_never_passes_a_match_that_completes_later(sim):
    """property (ii), outright and on the code's own `released` (word 1 of the row the sim wrote): after every prefix that ends in front
    of the hit's end, the released length is at most the start of the whole text's hit"""
    for k, stops_ in enumerate(STOP_SETS):
        tab = ref.table(stops_)
        stops = ref.live_stops(tab)
        cases = []
        for t in all_texts([b"a", b"b", b"c"], 6):
            f = ref.first_hit(t, stops)
            if f is not None:
                cases += [(t, c, f) for c in range(f[0])]
        _, _, rel = drive(sim, tab, [[(t[:c], False), (t[c:], False)] for t, c, _ in cases], geometry=GEOMETRIES[k % 4], three=(k % 2 == 0))
        for b, (t, c, f) in enumerate(cases):
            assert rel[0][b] <= f[1] and rel[1][b] == f[1], (stops_, t, c, rel[0][b])


# ------------------------------------------------------------------------------------------ 3. long stops, chunk and step edges
LONG = bytes(range(65, 65 + 64))                          # 64 different bytes


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_a_64_byte_stop_at_every_residue_and_cut(sim, geometry):
    """a 64-byte stop shifted through every residue of the chunk, the text cut at every step boundary"""
    tab = ref.table([LONG, b"zz"])
    feeds, want = [], []
    for shift in range(2 * geometry[1] + 2 if geometry[1] < 64 else 128):      # (every residue of the chunk, twice over)
        text = b"." * shift + LONG + b"tail"
        for c in range(len(text) + 1):                                         # (every step boundary)
            feeds.append([(text[:c], False), (text[c:], False)])
            want.append(b"." * shift)
    outs, hits, _ = drive(sim, tab, feeds, geometry=geometry, three=geometry[0] == 3)
    assert all(h == 0 for h in hits) and outs == want
    # ... and in pieces of 5 and of 64 bytes
    text = b"." * 70 + LONG
    for piece in (5, 64):
        n = (len(text) + piece - 1) // piece
        outs, hits, _ = drive(sim, tab, [[(text[i * piece:(i + 1) * piece], False) for i in range(n)]], geometry=geometry)
        assert outs == [b"." * 70] and hits == [0]


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_63_held_bytes_leave_at_once_on_a_mismatch(sim, geometry):
    tab = ref.table([LONG])
    feeds = []
    for shift in range(2 * geometry[1] + 2 if geometry[1] < 64 else 128):      # (every residue of the chunk, twice over)
        text = b"." * shift + LONG[:63]
        for c in range(len(text) + 1):                                         # (every step boundary)
            feeds.append([(text[:c], False), (text[c:], False), (b"!", False)])
    outs, hits, rel = drive(sim, tab, feeds, geometry=geometry)
    for f, o, h, b in zip(feeds, outs, hits, range(len(feeds))):
        text = f[0][0] + f[1][0]
        assert o == text + b"!" and h == -1
        assert rel[1][b] == len(text) - 63 and rel[2][b] == len(text) + 1      # 63 bytes held, then all of them leave at once


# ------------------------------------------------------------------------------------------ 4. masks, final, sticky, idle, include
def test_masks_and_dead_slots(sim):
    """a per-sequence subset of the slots; slots of length 0 or 65 never match"""
    tab = ref.table([b"ab", b"bc", b"c", b"a", b"b"], lens={3: 0, 4: 65})
    texts = [b"xabcx", b"xabcx", b"xabcx", b"xabcx", b"xabcx", b"aabb"]
    masks = [0b00001, 0b00010, 0b00100, 0b11000, 0, 0xFFFFFFFFFFFFFFFF]
    for three in (False, True):
        outs, hits, _ = drive(sim, tab, [[(t, False), (b"", True)] for t in texts], masks=masks, three=three)
        assert outs == [b"x", b"xa", b"xab", b"xabcx", b"xabcx", b"a"] and hits == [0, 1, 2, -1, -1, 0]


def test_final_for_a_subset_and_for_all(sim):
    tab = ref.table([b"abc"])
    texts = [b"xxab", b"xxab", b"ab", b"xabc"]
    for three in (False, True):
        outs, hits, rel = drive(sim, tab, [[(t, i in (0, 2)), (b"c", False)] for i, t in enumerate(texts)], three=three)
        # (a final closes the text: the "c" fed behind it does not complete "abc")
        assert outs == [b"xxabc", b"xx", b"abc", b"x"] and hits == [-1, 0, -1, 0]
        outs, hits, _ = drive(sim, tab, [[(t, False)] for t in texts], final_all=True, three=three)
        assert outs == [b"xxab", b"xxab", b"ab", b"x"] and hits == [-1, -1, -1, 0]


def test_stopped_is_sticky_and_idle_rows_stay_bit_for_bit(sim):
    tab = ref.table([b"ab"])
    seq = [(b"xab", False), (b"abab", False), (b"", True), (b"ab", True)]
    idle = [(b"xa", False), (b"", False), (b"", False), (b"", False)]
    for three in (False, True):
        for in_place in (False, True):
            drive(sim, tab, [seq, idle, seq], three=three, in_place=in_place)      # (rows against the oracle in every call)
    # the row of a stopped sequence and of one without new bytes, spelled out
    data, off = ref.csr([b"xab", b"xa"])
    _, _, hit, rows = sim.step(data, off, np.zeros((2, 10), dtype=np.uint64), tab, capacity=64)
    assert hit.tolist() == [0, -1] and rows[0, 0] == 3 | (1 << 16) and rows[0, 1] == 1 and rows[1, 0] == 2 | (1 << 8) and rows[1, 1] == 1
    data, off = ref.csr([b"zzzab", b""])
    out, o2, hit2, rows2 = sim.step(data, off, rows, tab, capacity=64)
    assert out == b"" and hit2.tolist() == [0, -1] and (rows2 == rows).all()


def test_include_releases_the_stop_itself(sim):
    for stops_ in STOP_SETS[:6]:
        tab = ref.table(stops_)
        texts = all_texts([b"a", b"b", b"c"], 5)
        outs, hits, _ = drive(sim, tab, [[(t[:2], False), (t[2:], False)] for t in texts], include=True, three=True)
        stops = ref.live_stops(tab)
        for t, o in zip(texts, outs):
            f = ref.first_hit(t, stops)
            assert o == (t[:f[0]] if f else t[:len(t) - ref.held(t, stops)])


def test_an_empty_batch_writes_the_closing_offset_and_nothing_else(sim):
    tab = ref.table([b"ab"])
    for three in (False, True):
        for geometry in GEOMETRIES:
            out, off, hit, rows = sim.step(b"", np.zeros(1, dtype=np.uint64), np.zeros((0, 10), dtype=np.uint64), tab, capacity=16,
                                           lanes=geometry[0], chunk=geometry[1], three=three)     # (step asserts the write counts)
            assert out == b"" and off.tolist() == [0] and hit.shape == (0,) and rows.shape == (0, 10)


# ------------------------------------------------------------------------------------------ 5. capacity, in place, clamped input
def test_the_capacity_cuts_bytes_only(sim):
    tab = ref.table([b"abc", b"bc"])
    texts = all_texts([b"a", b"b", b"c"], 4)
    full = drive(sim, tab, [[(t, False), (t, False)] for t in texts], check_rows=True)
    for cap in (0, 1, 17, 64):
        for three in (False, True):
            _, hits, rel = drive(sim, tab, [[(t, False), (t, False)] for t in texts], capacity=cap, three=three)
            assert hits == full[1] and all((a == b).all() for a, b in zip(rel, full[2]))


def test_state_in_place(sim):
    tab = ref.table([b"abca", b"bcab"])
    texts = all_texts([b"a", b"b", b"c"], 6)
    for three in (False, True):
        a = drive(sim, tab, [[(t[:3], False), (t[3:], False)] for t in texts], three=three, in_place=True)
        b = drive(sim, tab, [[(t[:3], False), (t[3:], False)] for t in texts], three=three)
        assert a[0] == b[0] and a[1] == b[1]


def test_input_offsets_beyond_the_capacity_are_clamped(sim):
    tab = ref.table([b"ab"])
    data = np.frombuffer(b"xxayyab!POISONPOISON", dtype=np.uint8)
    off = np.array([0, 3, 5, 100, 2 ** 40], dtype=np.uint64)      # capacity 8: sequence 2 is "ab!", sequence 3 is empty
    out, o, hit, rows = sim.step(data, off, np.zeros((4, 10), dtype=np.uint64), tab, capacity=64, in_capacity=8)
    assert out == b"xxyy" and o.tolist() == [0, 2, 4, 4, 4] and hit.tolist() == [-1, -1, 0, -1]
    assert rows[0, 0] == 3 | (1 << 8) and rows[3].tolist() == [0] * 10
    out, o, hit, rows = sim.step(data, off, np.zeros((4, 10), dtype=np.uint64), tab, capacity=64, in_capacity=0, three=True)
    assert out == b"" and (rows == 0).all() and hit.tolist() == [-1] * 4


# ------------------------------------------------------------------------------------------ 6. UTF-8
def test_every_released_piece_of_utf8_text_decodes(sim):
    """over {a, é, €, 😀} with stops of the same alphabet: every cut is a character boundary, whatever the BYTE cut of the steps'
    complete characters"""
    alpha = ["a", "é", "€", "😀"]
    tab = ref.table(["é€", "😀", "aé", "€€a"])
    texts = ["".join(t) for k in range(6) for t in itertools.product(alpha, repeat=k)]
    feeds = []
    for t in texts:
        for c in range(len(t) + 1):
            feeds.append([(t[:c].encode(), False), (t[c:].encode(), False), (b"", True)])
    B = len(feeds)
    state = np.zeros((B, 10), dtype=np.uint64)
    for c in range(3):
        data, off = ref.csr([f[c][0] for f in feeds])
        fin = np.array([1 if f[c][1] else 0 for f in feeds], dtype=np.uint8)
        out, o, _, state = sim.step(data, off, state, tab, final=fin, capacity=len(data) + 64 * B, three=(c == 1), lanes=5, chunk=3)
        for b in range(B):
            out[int(o[b]):int(o[b + 1])].decode("utf-8")               # (strict: raises on a cut inside a character)
    drive(sim, tab, feeds, geometry=(3, 2))


# ------------------------------------------------------------------------------------------ 7. the mutants
def test_mutant_front_halo_of_62_bytes_is_caught(sim):
    """a 64-byte stop that ends on a chunk's first position needs all 63 bytes in front of the chunk"""
    tab = ref.table([LONG])
    feeds = [[(b"." * shift + LONG, False)] for shift in range(0, 3)] + [[(LONG[:63], False), (LONG[63:], False)]]
    drive(sim, tab, feeds)
    with pytest.raises(AssertionError):
        drive(sim, tab, feeds, mutant="halo62")
    with pytest.raises(AssertionError):
        drive(sim, tab, feeds, mutant="halo62", geometry=(3, 2), three=True)


def test_mutant_shortest_at_equal_ends_is_caught(sim):
    """{abc, bc}: both end where "xabc" ends; the longest wins"""
    tab = ref.table([b"abc", b"bc"])
    feeds = [[(b"xabc", False)], [(b"xbc", False)]]
    outs, hits, _ = drive(sim, tab, feeds)
    assert outs == [b"x", b"x"] and hits == [0, 1]
    with pytest.raises(AssertionError):
        drive(sim, tab, feeds, mutant="shortest")
    # (where no two stops share an end the mutant is right: the check above is the one that names it)
    drive(sim, ref.table([b"ab", b"abc"]), [[(b"xabc", False)]], mutant="shortest")
