"""GPU tests (-m gpu) of the ragged all-gather's unpack launches at world sizes ABOVE one, on one GPU: a slab is data and an all-gather
leaves `world` slabs side by side, so the layout is built on the host (tests/gather_ref.py, written from the header) and copied to the
device as the collective would leave it.  What only runs when world > 1 -- the prefix loop over the other ranks' headers, who writes
the closing offset, the capacity checks relative to a nonzero base, the three-byte id format read behind a nonzero base, the running
totals of the wave form, the rebase of the exact form -- is compared bit for bit with the reference; every result buffer sits between
guard words.  What this cannot cover: RCCL itself, the links, and the overlap of streams at N > 1."""
import contextlib
import ctypes
import types

import numpy as np
import pytest

import gather_ref as G
from test_gpu_fused import oracle_csr            # (the oracle on sixteen threads, not one per CPU of the host)
from test_gpu_parity import _force_tiles, tok

pytestmark = pytest.mark.gpu

GUARD = 64
GUARD_WORD = {4: 0xA5A5A5A5, 8: 0xA5A5A5A5A5A5A5A5}
FILL_WORD = {4: 0x5A5A5A5A, 8: 0x5A5A5A5A5A5A5A5A}      # what a result buffer holds where nothing was written
FORMS = ["plain", "group", "at"]
DEPTH, NB = 3, 2                                         # the group form: a bucket of depth 3 holding two batches


def _dev():
    import torch
    return torch.device("cuda", 0)


def _stream():
    import torch
    return torch.cuda.current_stream(_dev()).cuda_stream


class Buf:
    """A result buffer as an interior view of a larger tensor: GUARD words of 0xA5.. on each side, the interior pre-filled."""

    def __init__(self, n, dtype, fill=None):
        import torch
        self.n, self.dtype = int(n), np.dtype(dtype)
        self.fill = FILL_WORD[self.dtype.itemsize] if fill is None else fill
        host = np.full(self.n + 2 * GUARD, GUARD_WORD[self.dtype.itemsize], dtype=self.dtype)
        host[GUARD:GUARD + self.n] = self.fill
        self.whole = torch.from_numpy(host.view(np.int32 if self.dtype.itemsize == 4 else np.int64)).to(_dev())
        self.init = self.whole.clone()
        self.t = self.whole[GUARD:GUARD + self.n]

    @property
    def ptr(self):
        return self.whole.data_ptr() + GUARD * self.dtype.itemsize

    def refill(self):
        self.whole.copy_(self.init)              # (device to device, in stream order)

    def get(self, whole=None):
        """the interior on the host (of `whole`: a copy of the tensor taken earlier); the guards must be as they were"""
        host = (self.whole if whole is None else whole).cpu().numpy().view(self.dtype)
        g = GUARD_WORD[self.dtype.itemsize]
        assert np.all(host[:GUARD] == g), f"written in front of the buffer: {np.flatnonzero(host[:GUARD] != g)[:8]}"
        assert np.all(host[GUARD + self.n:] == g), f"written behind the buffer: {np.flatnonzero(host[GUARD + self.n:] != g)[:8]}"
        return host[GUARD:GUARD + self.n].copy()


@contextlib.contextmanager
def slab_format(p24, handles=None):
    from splintr_amd import _ffi
    hs = handles or [tok("cl100k_base").handle]
    try:
        for h in hs:
            assert _ffi.lib().spl_set_option(h, b"slab_pack24", 1 if p24 else 0) == 0
        yield
    finally:
        for h in hs:
            assert _ffi.lib().spl_set_option(h, b"slab_pack24", 0) == 0


def _upload(slabs):
    import torch
    return torch.from_numpy(np.concatenate(slabs).view(np.int32)).to(_dev())


# ---------------------------------------------------------------------------------------------------------------------------------
# rank shapes
MAX_DOCS, MAX_TOKENS, MAX_LEN = 9, 200, 40


def _special_ids(p24):
    return [0xFFFFFF, 0, 0x010203, 0x800000] if p24 else [0xFFFFFFFF, 0, 0x010203, 0x80000000]


def make_rank(kind, rng, p24, idc, max_docs=MAX_DOCS, max_len=MAX_LEN):
    """(ids, off) of one rank.  kind: empty (N = 0), zero (documents, all empty), full (N = max_docs), cap (T = the slab's id capacity
    exactly), rand, res0 .. res3 (T mod 4 given: in the three-byte format the last id then ends at that byte alignment)"""
    if kind == "empty":
        lens = np.zeros(0, np.int64)
    elif kind == "zero":
        lens = np.zeros(int(rng.integers(1, max_docs + 1)), np.int64)
    elif kind == "cap":
        lens, left = [], idc
        for _ in range(max_docs):
            lens.append(min(max_len, left))
            left -= lens[-1]
        assert left == 0
        lens = np.array(lens, np.int64)
    else:
        n = max_docs if kind == "full" else int(rng.integers(2, max_docs))
        lens = rng.integers(0, max_len + 1, size=n)
        if lens.sum() > idc - 4:
            lens //= 2
        if kind.startswith("res"):                        # the last length is CHOSEN among those that give the residue and fit the slab
            rest = int(lens[:-1].sum())
            fits = [v for v in range(max_len + 1) if (rest + v) % 4 == int(kind[3]) and 0 < rest + v <= idc]
            assert fits, (kind, rest, idc, max_len)
            lens[-1] = fits[int(rng.integers(0, len(fits)))]
    assert int(lens.sum()) <= idc and len(lens) <= max_docs
    return rank_of_lens(lens, rng, p24)


def rank_of_lens(lens, rng, p24):
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    t = int(off[-1])
    ids = rng.integers(0, 1 << (24 if p24 else 32), size=t, dtype=np.uint64).astype(np.uint32)
    sp = _special_ids(p24)
    ids[:min(t, 4)] = sp[:min(t, 4)]
    if t >= 5:
        ids[-1] = sp[0]                          # all ones as the LAST id: what lies behind it in the slab must not leak in
    return ids, off


CASES_A = [
    (2, ["empty", "rand"]), (2, ["rand", "empty"]), (2, ["cap", "full"]), (2, ["zero", "res1"]), (2, ["res2", "res3"]), (2, ["res0", "cap"]),
    (3, ["rand", "empty", "rand"]), (3, ["res1", "res2", "res3"]), (3, ["cap", "zero", "full"]), (3, ["empty", "empty", "res0"]),
    (8, ["empty", "res1", "full", "res2", "empty", "zero", "res3", "empty"]),
    (8, ["cap", "res0", "rand", "res3", "res3", "res1", "full", "cap"]),
]


class Geometry:
    def __init__(self, world, p24, max_tokens=MAX_TOKENS, max_docs=MAX_DOCS):
        self.world, self.p24, self.max_docs = world, p24, max_docs
        self.cap_words = G.slab_words(max_tokens, max_docs, p24)
        self.idc = G.id_cap(self.cap_words, max_docs, p24)

    def slab(self, rank):
        return G.build_slab(rank[0], rank[1], self.cap_words, self.max_docs, self.p24)

    def garbage(self):
        return np.full(self.cap_words, G.FILL_WORD, dtype=np.uint32)


def run_form(form, geo, batches, all_ids_cap=None, all_off_cap=None):
    """One launch of `form` over batches[j][r] = (ids, off).  Returns ([(ids, off) per batch], status, run or None); the guards of every
    result buffer are checked on the way."""
    import torch
    from splintr_amd import _ffi
    L, h, w = _ffi.lib(), tok("cl100k_base").handle, geo.world
    ids_cap = all_ids_cap if all_ids_cap is not None else w * geo.idc
    off_cap = all_off_cap if all_off_cap is not None else w * geo.max_docs + 1
    status = Buf(1, np.uint32, fill=0)
    with slab_format(geo.p24):
        if form == "group":
            assert len(batches) == NB
            recv = _upload([geo.slab(batches[j][r]) if j < NB else geo.garbage() for r in range(w) for j in range(DEPTH)])
            a_ids, a_off = Buf(NB * ids_cap, np.uint32), Buf(NB * off_cap, np.uint64)
            rc = L.spl_gatherv_unpack_group(h, recv.data_ptr(), w, DEPTH, NB, geo.cap_words, geo.max_docs, a_ids.ptr, ids_cap, a_off.ptr,
                                            off_cap, status.ptr, _stream())
            run = None
        else:
            assert len(batches) == 1
            recv = _upload([geo.slab(rk) for rk in batches[0]])
            a_ids, a_off = Buf(ids_cap, np.uint32), Buf(off_cap, np.uint64)
            if form == "plain":
                rc = L.spl_gatherv_unpack(h, recv.data_ptr(), w, geo.cap_words, geo.max_docs, a_ids.ptr, ids_cap, a_off.ptr, status.ptr, _stream())
                run = None
            else:
                run = Buf(2, np.uint64, fill=0)
                rc = L.spl_gatherv_unpack_at(h, recv.data_ptr(), w, geo.cap_words, geo.max_docs, a_ids.ptr, ids_cap, a_off.ptr, off_cap,
                                             run.ptr, status.ptr, _stream())
        assert rc == 0, _ffi.last_error()
        torch.cuda.synchronize()
    g_ids, g_off = a_ids.get(), a_off.get()
    res = [(g_ids[j * ids_cap:(j + 1) * ids_cap], g_off[j * off_cap:(j + 1) * off_cap]) for j in range(len(batches))]
    return res, int(status.get()[0]), (run.get().tolist() if run is not None else None)


def check_batches(form, geo, batches):
    res, status, run = run_form(form, geo, batches)
    assert status == 0
    for (g_ids, g_off), ranks in zip(res, batches):
        w_ids, w_off = G.ref_unpack(ranks)
        # (offsets past the global document count + 1 and ids past the total are unspecified: not compared)
        assert np.array_equal(g_off[:len(w_off)], w_off), (g_off[:len(w_off)].tolist(), w_off.tolist())
        bad = np.flatnonzero(g_ids[:len(w_ids)] != w_ids)
        assert bad.size == 0, (bad[:8].tolist(), g_ids[bad[:8]].tolist(), w_ids[bad[:8]].tolist())
        if run is not None:
            assert run == [len(w_ids), len(w_off) - 1]


@pytest.mark.parametrize("p24", [False, True], ids=["u32", "pack24"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", range(len(CASES_A)), ids=[f"w{w}-{'-'.join(k)}" for w, k in CASES_A])
def test_every_form_and_format_at_world_2_3_8(case, form, p24):
    """A: empty ranks first, in the middle and last, a rank with max_docs documents, one with only empty documents, one filled to the
    slab's id capacity exactly (no overflow: status stays 0), every T mod 4 and ids with every byte set or clear."""
    world, kinds = CASES_A[case]
    geo = Geometry(world, p24)
    rng = np.random.default_rng(1000 + case)
    batches = [[make_rank(k, rng, p24, geo.idc) for k in kinds]]
    if form == "group":                                   # batch 1 of the bucket: other shapes at every rank
        batches.append([make_rank(k, rng, p24, geo.idc) for k in kinds[1:] + kinds[:1]])
    if "cap" in kinds:
        assert any(int(o[-1]) == geo.idc for _, o in batches[0])
    check_batches(form, geo, batches)


@pytest.mark.parametrize("p24", [False, True], ids=["u32", "pack24"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("big_first", [True, False])
def test_stride_loops_go_round_twice(big_first, form, p24):
    """B: 70 000 ids and 40 000 documents in one rank -- the unpack grid is 128 x 256 threads per rank, so both stride loops repeat."""
    geo = Geometry(2, p24, max_tokens=70000, max_docs=40000)
    rng = np.random.default_rng(7)

    def big():
        lens = rng.multinomial(70000, np.full(40000, 1.0 / 40000))
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        return rng.integers(0, 1 << (24 if p24 else 32), size=70000, dtype=np.uint64).astype(np.uint32), off

    def small():
        return make_rank("res3", rng, p24, geo.idc, max_docs=5, max_len=6)

    batches = [[big(), small()] if big_first else [small(), big()] for _ in range(NB if form == "group" else 1)]
    check_batches(form, geo, batches)


def _tiny_ranks(rng, p24, world):
    """at most two documents and five ids per rank; about a third of the ranks have no document"""
    shapes = [[], [], [0], [2], [0, 0], [1, 2], [3, 2], [0, 4]]
    return [rank_of_lens(np.array(shapes[int(rng.integers(0, len(shapes)))], np.int64), rng, p24) for _ in range(world)]


@pytest.mark.parametrize("p24", [False, True], ids=["u32", "pack24"])
@pytest.mark.parametrize("form", ["plain", "at"])
def test_world_64(form, p24):
    """C: the largest communicator (COMM_MAX_WORLD): 64 headers in the prefix loop and in the advance."""
    geo = Geometry(64, p24, max_tokens=5, max_docs=2)
    rng = np.random.default_rng(64)
    if form == "plain":
        ranks = _tiny_ranks(rng, p24, 64)
        ranks[0], ranks[63] = make_rank("empty", rng, p24, 5), rank_of_lens(np.array([3, 2]), rng, p24)
        check_batches("plain", geo, [ranks])
        return
    waves = [_tiny_ranks(rng, p24, 64) for _ in range(2)]
    waves[1][0], waves[1][63] = make_rank("empty", rng, p24, 5), make_rank("empty", rng, p24, 5)
    check_waves(geo, waves, [[0, 1]])


# ---------------------------------------------------------------------------------------------------------------------------------
# D: overflow
@pytest.mark.parametrize("p24", [False, True], ids=["u32", "pack24"])
@pytest.mark.parametrize("form", ["plain", "group"])
def test_a_slab_that_overflowed_is_reported_and_contained(form, p24):
    """The middle rank of three claims one id more than its slab carries: status 1, and because the bases use the CLAIMED T the other
    ranks' ids and every offset are where they belong."""
    geo = Geometry(3, p24)
    rng = np.random.default_rng(31)
    batches = []
    for _ in range(NB if form == "group" else 1):
        over_off = np.array([0, 40, 40, geo.idc + 1], np.uint64)
        over = (rng.integers(0, 1 << 24, size=geo.idc + 1, dtype=np.uint64).astype(np.uint32), over_off)
        batches.append([make_rank("res1", rng, p24, geo.idc), over, make_rank("full", rng, p24, geo.idc)])
    res, status, _ = run_form(form, geo, batches, all_ids_cap=3 * (geo.idc + 1))
    assert status == 1
    for (g_ids, g_off), ranks in zip(res, batches):
        w_ids, w_off = G.ref_unpack(ranks)
        assert np.array_equal(g_off[:len(w_off)], w_off)
        t0, t1 = int(ranks[0][1][-1]), int(ranks[1][1][-1])
        assert np.array_equal(g_ids[:t0], w_ids[:t0]) and np.array_equal(g_ids[t0 + t1:len(w_ids)], w_ids[t0 + t1:])
        # the ids the full slab does carry (its id area used up to the slack word) are delivered
        assert np.array_equal(g_ids[t0:t0 + geo.idc], ranks[1][0][:geo.idc])
    if form == "group":                                   # only batch 1 overflows: still reported
        batches[0][1] = make_rank("rand", rng, p24, geo.idc)
        assert run_form(form, geo, batches, all_ids_cap=3 * (geo.idc + 1))[1] == 1


def check_waves(geo, waves, orders, ids_cap=None, off_cap=None, expect_status=0, slack=0):
    """spl_gatherv_unpack_at once per wave on ONE stream with no host synchronisation in between, on one zeroed d_run; for every order
    in `orders` (run zeroed on the same stream in between, as WaveGather.begin does).  The buffers are `slack` entries longer than the
    capacities the call is given: what lies at or beyond a capacity must keep its fill."""
    import torch
    from splintr_amd import _ffi
    L, h, w = _ffi.lib(), tok("cl100k_base").handle, geo.world
    t_tot = sum(int(o[-1]) for wave in waves for _, o in wave)
    n_tot = sum(len(o) - 1 for wave in waves for _, o in wave)
    ids_cap = t_tot if ids_cap is None else ids_cap
    off_cap = n_tot + 1 if off_cap is None else off_cap
    recv = [_upload([geo.slab(rk) for rk in wave]) for wave in waves]
    a_ids, a_off = Buf(ids_cap + slack, np.uint32), Buf(off_cap + slack, np.uint64)
    run, status = Buf(2, np.uint64, fill=0), Buf(1, np.uint32, fill=0)
    got = []
    with slab_format(geo.p24):
        for i, order in enumerate(orders):
            if i:
                for b in (a_ids, a_off, status):
                    b.refill()
                run.t.zero_()
            for k in order:
                rc = L.spl_gatherv_unpack_at(h, recv[k].data_ptr(), w, geo.cap_words, geo.max_docs, a_ids.ptr, ids_cap, a_off.ptr, off_cap,
                                             run.ptr, status.ptr, _stream())
                assert rc == 0, _ffi.last_error()
            got.append(tuple(b.whole.clone() for b in (a_ids, a_off, run, status)))     # (a copy in stream order: nothing waits here)
        torch.cuda.synchronize()
    for order, snap in zip(orders, got):
        g_ids, g_off, g_run, g_status = (b.get(s) for b, s in zip((a_ids, a_off, run, status), snap))
        w_ids, w_off, w_run, w_status, m_ids, m_off = G.ref_unpack_waves([waves[k] for k in order], ids_cap, off_cap, id_cap=geo.idc)
        assert w_status == expect_status and int(g_status[0]) == w_status
        assert g_run.tolist() == w_run == [t_tot, n_tot]
        assert np.array_equal(g_ids[:ids_cap][m_ids], w_ids[m_ids]), order
        assert np.array_equal(g_off[:off_cap][m_off], w_off[m_off]), (order, g_off[:off_cap].tolist(), w_off.tolist())
        if expect_status == 0:
            assert m_ids.all() and m_off.all()
        assert np.all(g_ids[ids_cap:] == a_ids.fill) and np.all(g_off[off_cap:] == a_off.fill)


@pytest.mark.parametrize("p24", [False, True], ids=["u32", "pack24"])
@pytest.mark.parametrize("cut", ["ids", "off"])
def test_wave_form_overflow_of_a_result_buffer(cut, p24):
    """D, wave form: the result buffer ends in the middle of wave 1's rank 1 -- (a) its ids, (b) its documents.  Status 1, everything
    below the capacity as the reference has it, nothing at or beyond it, run = the claimed totals."""
    geo = Geometry(3, p24)
    rng = np.random.default_rng(41)
    waves = [[make_rank(k, rng, p24, geo.idc) for k in kinds] for kinds in (["res1", "zero", "res2"], ["rand", "full", "res3"])]
    t_before = sum(int(o[-1]) for _, o in waves[0]) + int(waves[1][0][1][-1])
    n_before = sum(len(o) - 1 for _, o in waves[0]) + len(waves[1][0][1]) - 1
    t_r, n_r = int(waves[1][1][1][-1]), len(waves[1][1][1]) - 1
    assert t_r >= 2 and n_r >= 2
    if cut == "ids":
        check_waves(geo, waves, [[0, 1]], ids_cap=t_before + t_r // 2, expect_status=1, slack=600)
    else:
        check_waves(geo, waves, [[0, 1]], off_cap=n_before + n_r // 2, expect_status=1, slack=40)


@pytest.mark.parametrize("p24", [False, True], ids=["u32", "pack24"])
@pytest.mark.parametrize("world,n_waves,first_empty", [(2, 1, False), (2, 1, True), (3, 3, False), (3, 3, True), (8, 8, False), (8, 8, True)])
def test_waves_in_stream_order(world, n_waves, first_empty, p24):
    """E: n_waves calls behind each other, the running totals carried in device memory; one wave in which every rank is empty (wave 0
    in one parametrisation); then the totals zeroed on the same stream and the waves again in another order."""
    geo = Geometry(world, p24)
    rng = np.random.default_rng(500 + 10 * world + n_waves)
    kinds = ["empty", "zero", "full", "rand", "res0", "res1", "res2", "res3", "cap"]
    waves = [[make_rank(str(rng.choice(kinds)), rng, p24, geo.idc) for _ in range(world)] for _ in range(n_waves)]
    hole = 0 if first_empty else (n_waves // 2 if n_waves > 1 else None)
    if hole is not None:
        waves[hole] = [make_rank("empty", rng, p24, geo.idc) for _ in range(world)]
    fwd = list(range(n_waves))
    check_waves(geo, waves, [fwd, fwd[::-1] if n_waves > 1 else fwd])


# ---------------------------------------------------------------------------------------------------------------------------------
# F, G: the real encoder at simulated world sizes
class Plans:
    """The two real batches, their oracle CSRs and the DeviceBatches of every slice of a wave plan, made once per module and released
    with it."""

    def __init__(self, coracle):
        self.coracle, self.batches, self.plans = coracle, {}, {}

    def real_batch(self, n_docs):
        """(texts, oracle ids, oracle offsets) of corpus.c2(n_docs, seed=5) with every 17th text emptied; encoded by the oracle once"""
        if n_docs not in self.batches:
            from splintr_amd import corpus
            texts = ["" if i % 17 == 0 else t for i, t in enumerate(corpus.c2(n_docs, seed=5))]
            self.batches[n_docs] = (texts,) + tuple(oracle_csr(self.coracle("cl100k_base"), texts))
        return self.batches[n_docs]

    def wave_plan(self, n_docs, world, n_waves, taper):
        """plan_waves over the batch, a DeviceBatch per slice (k, r) -- empty slices included -- and the slab geometry that fits every slice"""
        key = (n_docs, world, n_waves, taper)
        if key not in self.plans:
            from splintr_amd.device import DeviceBatch, reserve
            from splintr_amd.distributed import plan_waves
            texts, _, o_off = self.real_batch(n_docs)
            pw = plan_waves([len(t.encode("utf-8")) for t in texts], world, n_waves, taper)
            dbs = [[DeviceBatch(texts[lo:hi], _dev()) for lo, hi in wave] for wave in pw]
            max_docs = max(1, max(hi - lo for wave in pw for lo, hi in wave))
            max_tokens = max(int(o_off[hi] - o_off[lo]) for wave in pw for lo, hi in wave)
            reserve(tok("cl100k_base"), max(b.n_bytes for row in dbs for b in row), max_docs)
            self.plans[key] = (pw, dbs, max_docs, max_tokens)
        return self.plans[key]


@pytest.fixture(scope="module")
def plans(coracle):
    p = Plans(coracle)
    yield p
    p.batches.clear(), p.plans.clear()


def encode_slices(handle, dbs, geo, only=None):
    """slice (k, r) straight into recv[k][r * cap_words:] by the packed encode; slabs nobody writes keep a pattern no header survives"""
    import torch
    from splintr_amd import _ffi
    L = _ffi.lib()
    recv = [torch.full((geo.world * geo.cap_words,), 0x5A5A5A5A, dtype=torch.int32, device=_dev()) for _ in dbs]
    for k, row in enumerate(dbs):
        for r, b in enumerate(row):
            if only is not None and not only(k, r):
                continue
            rc = L.spl_encode_batch_device_packed(handle, b.text.data_ptr(), b.n_bytes, b.doc_off.data_ptr(), b.n_docs, 0, b.ids.data_ptr(),
                                                  b.ids.numel(), b.out_off.data_ptr(), recv[k][r * geo.cap_words:].data_ptr(), geo.cap_words,
                                                  geo.max_docs, _stream())
            assert rc == 0, f"slice ({k}, {r}) of {b.n_docs} documents, {b.n_bytes} bytes: {_ffi.last_error()}"
    return recv


@pytest.mark.parametrize("geom", [0, 4], ids=["tile", "queue"])
@pytest.mark.parametrize("p24", [False, True], ids=["u32", "pack24"])
@pytest.mark.parametrize("n_docs", [300, 40])
@pytest.mark.parametrize("world,n_waves,taper", [(2, 3, 0.85), (8, 8, 0.85), (3, 5, 0.6)])
def test_real_encoder_at_simulated_worlds(plans, world, n_waves, taper, n_docs, p24, geom):
    """F: every slice of plan_waves encoded by spl_encode_batch_device_packed into its place of the receive buffer (in geometry 0 the
    tile kernel writes the slab, in 4 the pack kernel), unpacked wave by wave: the oracle's CSR of the whole batch.  With 40
    documents at 8 x 8, 25 of the 64 slices are EMPTY (no documents at all): their slabs must say so."""
    import torch
    from splintr_amd import _ffi
    texts, o_ids, o_off = plans.real_batch(n_docs)
    pw, dbs, max_docs, max_tokens = plans.wave_plan(n_docs, world, n_waves, taper)
    if (n_docs, world, n_waves) == (40, 8, 8):
        assert sum(1 for wave in pw for lo, hi in wave if lo == hi) == 25
    geo = Geometry(world, p24, max_tokens=max_tokens, max_docs=max_docs)
    L, h = _ffi.lib(), tok("cl100k_base").handle
    a_ids, a_off = Buf(len(o_ids), np.uint32), Buf(len(texts) + 1, np.uint64)
    run, status = Buf(2, np.uint64, fill=0), Buf(1, np.uint32, fill=0)
    _force_tiles("cl100k_base", geom)
    try:
        with slab_format(p24):
            recv = encode_slices(h, dbs, geo)
            for k in range(n_waves):
                rc = L.spl_gatherv_unpack_at(h, recv[k].data_ptr(), world, geo.cap_words, geo.max_docs, a_ids.ptr, a_ids.n, a_off.ptr, a_off.n,
                                             run.ptr, status.ptr, _stream())
                assert rc == 0, _ffi.last_error()
            torch.cuda.synchronize()
    finally:
        _force_tiles("cl100k_base", 0)
    assert int(status.get()[0]) == 0 and run.get().tolist() == [len(o_ids), len(texts)]
    assert np.array_equal(a_off.get(), o_off)
    assert np.array_equal(a_ids.get(), o_ids)


def _sim_wave_gather(world, rank, peers, **kw):
    import torch
    from splintr_amd.device import WaveGather

    class Sim(WaveGather):
        """this process is `rank`; the other ranks' slabs of wave k come from `peers[k]`, copied in on the exchange stream where the
        collective would deliver them"""

        def _allgather(self, k):
            assert torch.cuda.current_stream(self.dev).cuda_stream == self.exch.cuda_stream
            dst = self.recv[k].view(self.world, self.cap_words)
            for r in range(self.world):
                dst[r].copy_(self.send[k] if r == rank else peers[k].view(self.world, self.cap_words)[r])

    return Sim(comm=types.SimpleNamespace(world=world, handle=None), **kw)


@pytest.mark.parametrize("world,rank,p24,two", [(3, 0, False, False), (3, 0, True, False), (3, 2, False, False), (3, 2, True, True),
                                                (8, 0, False, False), (8, 0, True, False), (8, 7, False, False), (8, 7, True, False)])
def test_wave_gather_as_one_rank_of_a_larger_world(plans, world, rank, p24, two):
    """G: WaveGather itself -- its streams, events and its own encode -- as rank 0 and as the last rank of 3 and 8, the other ranks' slabs
    supplied through the _allgather seam; finish() gives the oracle's CSR and totals, twice in a row (`two`: with tok2=, two encode streams)."""
    import torch
    from splintr_amd import Tokenizer
    n_waves = 4
    texts, o_ids, o_off = plans.real_batch(300)
    pw, dbs, max_docs, max_tokens = plans.wave_plan(300, world, n_waves, 0.85)
    geo = Geometry(world, p24, max_tokens=max_tokens, max_docs=max_docs)
    t = tok("cl100k_base")
    t2 = Tokenizer.from_pretrained("cl100k_base") if two else None
    handles = [t.handle] + ([t2.handle] if two else [])
    with slab_format(p24, handles):
        peers = encode_slices(t.handle, dbs, geo, only=lambda k, r: r != rank)
        wg = _sim_wave_gather(world, rank, peers, tok=t, device=_dev(), n_waves=n_waves, max_docs=max_docs, max_tokens=max_tokens,
                              total_tokens_cap=len(o_ids), total_docs_cap=len(texts), pack24=p24, tok2=t2)
        assert wg.cap_words == geo.cap_words and wg.world == world
        for _ in range(2):
            wg.begin()
            for k in range(n_waves):
                wg.encode_and_submit(dbs[k][rank])
            a_ids, a_off, run = wg.finish()
            torch.cuda.synchronize()
            assert not wg.overflowed() and run.cpu().tolist() == [len(o_ids), len(texts)]
            assert np.array_equal(a_off.cpu().numpy().astype(np.uint64), o_off)
            assert np.array_equal(a_ids.cpu().numpy().view(np.uint32), o_ids)
            a_ids.fill_(-1), a_off.fill_(-1)             # (the second round has to write all of it again)


# ---------------------------------------------------------------------------------------------------------------------------------
# H: the exact form's device side
@pytest.mark.parametrize("world", [2, 3, 8, 64])
def test_rebase_offsets_of_the_exact_form(world):
    """k_rebase_offsets through spl_debug_rebase_offsets (the function spl_allgatherv_csr calls): every rank's local offsets, laid side
    by side as the receives leave them, become global ones; the last rank writes the closing entry.  One rank has no document, one has
    300 000 -- more than the 1024 x 256 threads of the grid's cap, so the stride loop repeats."""
    import torch
    from splintr_amd import _ffi
    rng = np.random.default_rng(80 + world)
    n_docs = [int(n) for n in rng.integers(1, 20, size=world)]
    n_docs[int(rng.integers(0, world))] = 0
    big = next(r for r in (world - 1, 0) if n_docs[r])   # (not the empty one)
    n_docs[big] = 300000
    ranks = []
    for n in n_docs:
        off = np.concatenate([[0], np.cumsum(rng.integers(0, 4, size=n))]).astype(np.uint64)
        ranks.append((np.zeros(int(off[-1]), np.uint32), off))
    _, w_off = G.ref_unpack(ranks)
    a_off = Buf(len(w_off), np.uint64)
    host = np.full(len(w_off), a_off.fill, np.uint64)
    pre = 0
    for _, off in ranks:
        host[pre:pre + len(off) - 1] = off[:-1]
        pre += len(off) - 1
    a_off.t.copy_(torch.from_numpy(host.view(np.int64)))
    counts = (ctypes.c_uint64 * (2 * world))(*[v for _, off in ranks for v in (int(off[-1]), len(off) - 1)])
    rc = _ffi.lib().spl_debug_rebase_offsets(tok("cl100k_base").handle, a_off.ptr, counts, world, _stream())
    assert rc == 0, _ffi.last_error()
    torch.cuda.synchronize()
    got = a_off.get()
    bad = np.flatnonzero(got != w_off)
    assert bad.size == 0, (bad[:8].tolist(), got[bad[:8]].tolist(), w_off[bad[:8]].tolist())
