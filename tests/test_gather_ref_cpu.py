"""CPU tests of tests/gather_ref.py, the numpy statement of the ragged all-gather's wire format that the GPU tests of the unpack
kernels (test_gpu_gather_worlds.py) are compared against: the reference itself has to be right first."""
import os
import socket
import sys

import numpy as np
import pytest

import gather_ref as G
from conftest import ROOT


def _rank(rng, n_docs, max_len, id_hi):
    lens = rng.integers(0, max_len + 1, size=n_docs)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return rng.integers(0, id_hi, size=int(off[-1]), dtype=np.uint64).astype(np.uint32), off


@pytest.mark.parametrize("p24", [False, True])
def test_build_and_parse_round_trip(p24):
    rng = np.random.default_rng(3)
    max_docs = 4
    for t in range(10):                                  # T = 0 .. 9: every T mod 4, the empty rank, one id
        for n in (0, 1, 3, 4):
            if n == 0 and t:
                continue
            cuts = np.sort(rng.integers(0, t + 1, size=max(n - 1, 0)))
            off = np.concatenate([[0], cuts, [t]]).astype(np.uint64) if n else np.zeros(1, np.uint64)
            ids = rng.integers(0, 1 << (24 if p24 else 32), size=t, dtype=np.uint64).astype(np.uint32)
            cap = G.slab_words(9, max_docs, p24)
            slab = G.build_slab(ids, off, cap, max_docs, p24)
            assert slab.dtype == np.uint32 and len(slab) == cap and (int(slab[0]), int(slab[1])) == (t, n)
            g_ids, g_off = G.parse_slab(slab, max_docs, p24)
            assert np.array_equal(g_ids, ids) and np.array_equal(g_off, off)
            # what nothing was written to keeps the pattern: the offsets beyond N + 1, and the id area behind the last id
            assert np.all(slab[2 + n + 1:G.ids_at(max_docs)] == G.FILL_WORD)
            used = 3 * t if p24 else 4 * t
            assert np.all(slab[G.ids_at(max_docs):].view(np.uint8)[used:] == 0xC3)


def test_pack24_byte_layout_is_little_endian():
    slab = G.build_slab([0x010203, 0xA0B0C0], [0, 2], G.slab_words(2, 1, True), 1, True)
    assert slab[G.ids_at(1):].view(np.uint8)[:6].tolist() == [0x03, 0x02, 0x01, 0xC0, 0xB0, 0xA0]
    assert G.ids_at(1) == 4 and slab[:4].tolist() == [2, 1, 0, 2]
    u32 = G.build_slab([0x010203], [0, 1], G.slab_words(1, 1, False), 1, False)
    assert u32[G.ids_at(1)] == 0x010203


def test_slab_words_is_the_products_and_holds_max_tokens():
    from splintr_amd.device import _slab_words
    for p24 in (False, True):
        slack = set()
        for d in (0, 1, 7):
            for m in range(3001):
                w = G.slab_words(m, d, p24)
                assert w == _slab_words(m, d, p24)
                slack.add(G.id_cap(w, d, p24) - m)
        # a slab made for m ids carries a little MORE: "T equals the capacity" is id_cap, not max_tokens
        assert slack == ({1, 2} if p24 else {1})


def test_a_slab_longer_than_its_capacity_keeps_the_claim():
    cap = G.slab_words(4, 2, True)
    k = G.id_cap(cap, 2, True)
    ids = np.arange(k + 1, dtype=np.uint32)
    slab = G.build_slab(ids, [0, k + 1], cap, 2, True)
    g_ids, g_off = G.parse_slab(slab, 2, True)
    assert int(slab[0]) == k + 1 and g_off.tolist() == [0, k + 1] and np.array_equal(g_ids, ids[:k])
    assert 3 * k <= 4 * (cap - G.ids_at(2) - 1) and slab[-1] == G.FILL_WORD      # the ids stop in front of the slack word


def test_waves_without_overflow_equal_the_flat_unpack():
    rng = np.random.default_rng(11)
    for world, n_waves in ((1, 1), (2, 3), (3, 2), (8, 4)):
        waves = [[_rank(rng, int(rng.integers(0, 5)), 6, 1 << 32) for _ in range(world)] for _ in range(n_waves)]
        waves[n_waves // 2] = [(np.zeros(0, np.uint32), np.zeros(1, np.uint64)) for _ in range(world)]      # a wave nobody has anything in
        f_ids, f_off = G.ref_unpack([rk for w in waves for rk in w])
        ids, off, run, status, m_ids, m_off = G.ref_unpack_waves(waves, len(f_ids) + 5, len(f_off) + 3)
        assert status == 0 and run == [len(f_ids), len(f_off) - 1]
        assert np.array_equal(ids[:len(f_ids)], f_ids) and np.array_equal(off[:len(f_off)], f_off)
        assert m_ids.tolist() == [True] * len(f_ids) + [False] * 5 and m_off.tolist() == [True] * len(f_off) + [False] * 3
        # exactly fitting buffers are no overflow; one entry less of either is
        assert G.ref_unpack_waves(waves, len(f_ids), len(f_off))[3] == 0
        assert G.ref_unpack_waves(waves, len(f_ids), len(f_off) - 1)[3] == 1
        if len(f_ids):
            assert G.ref_unpack_waves(waves, len(f_ids) - 1, len(f_off))[3] == 1


def test_wave_overflow_is_contained_and_run_counts_the_claims():
    a = (np.array([1, 2, 3], np.uint32), np.array([0, 1, 3], np.uint64))
    b = (np.array([4, 5, 6, 7], np.uint32), np.array([0, 4], np.uint64))
    ids, off, run, status, m_ids, m_off = G.ref_unpack_waves([[a, b], [b, a]], 9, 5)
    assert status == 1 and run == [14, 6]
    assert ids.tolist() == [1, 2, 3, 4, 5, 6, 7, 4, 5] and m_ids.all()
    assert off.tolist() == [0, 1, 3, 7, 11] and m_off.all()
    # a rank that claims more than its slab carries: the ranks behind it still land where the claim puts them
    c = (np.array([9, 9, 9], np.uint32), np.array([0, 4], np.uint64))
    ids, off, run, status, m_ids, _ = G.ref_unpack_waves([[c, a]], 9, 8, id_cap=3)
    assert status == 1 and run == [7, 3] and off[:4].tolist() == [0, 4, 5, 7]
    assert ids[:7].tolist() == [9, 9, 9, 0, 1, 2, 3] and m_ids.tolist() == [True, True, True, False, True, True, True, False, False]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _stub_encode(local):
    """a stand-in for the encoder: one id per byte, so ragged and empty documents stay what they are"""
    rows = [np.frombuffer(t.encode("utf-8"), dtype=np.uint8).astype(np.uint32) + np.uint32(1000) for t in local]
    off = np.zeros(len(rows) + 1, dtype=np.uint64)
    if rows:
        np.cumsum([len(r) for r in rows], out=off[1:])
    return (np.concatenate(rows) if rows else np.zeros(0, np.uint32)).astype(np.uint32), off


_TEXTS = ["alpha", "", "be ta", "c" * 40, "", "", "delta delta", "e", "f" * 17, "", "gamma"] * 3


def _waves_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from splintr_amd.distributed import encode_batch_waves, plan_waves
    import gather_ref as G
    ok = True
    lens = [len(t.encode("utf-8")) for t in _TEXTS]
    for n_waves, taper in ((1, 1.0), (4, 1.0), (7, 0.6)):
        got_ids, got_off = encode_batch_waves(_stub_encode, _TEXTS, torch.device("cpu"), n_waves=n_waves, taper=taper)
        pw = plan_waves(lens, world, n_waves, taper)
        waves = [[_stub_encode(_TEXTS[lo:hi]) for lo, hi in wave] for wave in pw]
        ids, off, run, status, _, _ = G.ref_unpack_waves(waves, sum(lens), len(_TEXTS) + 1)
        ok = ok and status == 0 and run == [sum(lens), len(_TEXTS)] and np.array_equal(got_ids, ids) and np.array_equal(got_off, off)
    q.put((rank, bool(ok)))
    dist.destroy_process_group()


def test_waves_equal_encode_batch_waves_on_gloo():
    """splintr_amd.distributed.encode_batch_waves -- the host-tensor form of WaveGather -- with a stub encoder at world 2 gives what
    ref_unpack_waves gives for the slices plan_waves cuts."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_waves_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = [q.get(timeout=120) for _ in ps]
    for p in ps:
        p.join(timeout=60)
    assert all(ok for _, ok in res), res
