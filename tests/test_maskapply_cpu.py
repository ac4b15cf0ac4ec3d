"""The bitmask-to-logits kernel without a GPU: the index arithmetic of splintr_amd/csrc/spl_k_maskapply.h -- which columns a 16-byte piece
of an unaligned row holds, where head and tail are -- and the lane's decision, evaluated by tests/hostsim/maskapply_sim.cpp over counted
buffers against numpy on the bit patterns: nothing outside a row's columns is written, no byte twice, a byte that keeps its value is only
stored by a lane that loaded it first, the mask rows of rows that are not live are not read."""
import numpy as np
import pytest

COLS = [1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 255, 257, 1000]


@pytest.fixture(scope="module")
def sim():
    import maskapply_sim
    maskapply_sim.lib()
    return maskapply_sim


def test_pieces_by_hand(sim):
    # bf16, the row begins 3 elements behind a boundary, 20 masked columns: pieces of 5, 8 and 7 columns
    A = 0x1000 + 6
    assert sim.piece(A, 2, 20, 0) == dict(addr=0x1000, c0=0, j0=3, n=5, n_pieces=3)
    assert sim.piece(A, 2, 20, 1) == dict(addr=0x1010, c0=5, j0=0, n=8, n_pieces=3)
    assert sim.piece(A, 2, 20, 2) == dict(addr=0x1020, c0=13, j0=0, n=7, n_pieces=3)
    assert sim.piece(A, 2, 20, 3)["n"] == 0
    # f32, aligned, 4 columns: one whole piece; 1 column behind 3 elements: the last element of piece 0
    assert sim.piece(0x2000, 4, 4, 0) == dict(addr=0x2000, c0=0, j0=0, n=4, n_pieces=1)
    assert sim.piece(0x200C, 4, 1, 0) == dict(addr=0x2000, c0=0, j0=3, n=1, n_pieces=1)
    assert sim.piece(0x200C, 4, 2, 1) == dict(addr=0x2010, c0=1, j0=0, n=1, n_pieces=2)
    assert sim.piece(0x2000, 4, 0, 0)["n_pieces"] == 0


@pytest.mark.parametrize("es", [2, 4])
def test_pieces_tile_every_row(sim, es):
    """every column of a row is in exactly one piece, at its own address, and the grid covers the row's pieces"""
    E = 16 // es
    for a in range(E):
        A = 0x4000 + a * es
        for n_eff in [1, 2, E - 1, E, E + 1, 2 * E, 33, 100]:
            n_pieces = sim.piece(A, es, n_eff, 0)["n_pieces"]
            assert n_pieces <= sim.lib().ma_sim_grid_pieces(es, n_eff)
            seen = []
            for p in range(n_pieces + 2):
                q = sim.piece(A, es, n_eff, p)
                assert q["addr"] == (A & ~15) + 16 * p
                for i in range(q["n"]):
                    assert q["addr"] + (q["j0"] + i) * es == A + (q["c0"] + i) * es
                seen += list(range(q["c0"], q["c0"] + q["n"]))
                assert (q["n"] > 0) == (p < n_pieces)
            assert seen == list(range(n_eff))


def _vals(rng, dtype, sim, R, stride):
    v = rng.integers(0, 1 << (8 * sim.ELEM[dtype]), size=(R, stride), dtype=np.uint64).astype(sim.UINT[dtype])
    if v.size >= 4:                                        # NaN with a payload, +inf, -inf, -0.0
        special = {sim.F32: [0x7FC12345, 0x7F800000, 0xFF800000, 0x80000000], sim.F16: [0x7E01, 0x7C00, 0xFC00, 0x8000],
                   sim.BF16: [0x7FC1, 0x7F80, 0xFF80, 0x8000]}[dtype]
        v.reshape(-1)[:4] = special
    return v


def _masks(rng, R, n_words):
    """name -> uint32 [R, n_words]: all ones, all zeros, random, and exactly one 0 / one 1 bit at every position of two adjacent words"""
    out = {"ones": np.full((R, n_words), 0xFFFFFFFF, dtype=np.uint32), "zeros": np.zeros((R, n_words), dtype=np.uint32),
           "random": rng.integers(0, 1 << 32, size=(R, n_words), dtype=np.uint64).astype(np.uint32)}
    return out


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_apply_against_numpy(sim, dtype):
    rng = np.random.default_rng(dtype + 1)
    kinds = np.zeros(4, dtype=np.int64)
    for n_cols in COLS:
        for pad in (0, 5):
            for base in (0, 1):
                for R in (1, 3):
                    for n_words in sorted({max(1, (n_cols + 31) // 32 - 1), (n_cols + 31) // 32, (n_cols + 31) // 32 + 1}):
                        vals = _vals(rng, dtype, sim, R, n_cols + pad)
                        for name, mask in _masks(rng, R, n_words).items():
                            got, k = sim.run(vals, dtype, mask, n_cols=n_cols, base_elems=base)
                            assert (got == sim.expected(vals, dtype, mask, None, n_cols)).all(), (n_cols, pad, base, R, n_words, name)
                            kinds += k
                            if name == "ones":
                                assert (got == vals).all() and k[1:] == [0, 0, 0]
    assert (kinds > 0).all()                               # every kind of lane was met: nothing, store, load and store, element stores


@pytest.mark.parametrize("dtype", [1, 0])
def test_single_bits_across_two_words(sim, dtype):
    """exactly one 0 bit, and exactly one 1 bit, at every position of two adjacent words; rows on odd boundaries"""
    rng = np.random.default_rng(9)
    n_cols, R = 97, 64
    vals = _vals(rng, dtype, sim, R, n_cols)
    for one in (False, True):
        mask = np.zeros((R, 4), dtype=np.uint32) if one else np.full((R, 4), 0xFFFFFFFF, dtype=np.uint32)
        for r in range(R):
            mask[r, 1 + r // 32] ^= np.uint32(1 << (r % 32))
        for base in (0, 3):
            got, _ = sim.run(vals, dtype, mask, n_cols=n_cols, base_elems=base)
            assert (got == sim.expected(vals, dtype, mask, None, n_cols)).all(), (one, base)
            hit = (got != vals).sum(1)
            assert (hit <= (1 if not one else n_cols)).all()


def test_live_rows_and_mask_stride(sim):
    rng = np.random.default_rng(4)
    R, n_cols, n_words = 9, 77, 3
    vals = _vals(rng, sim.BF16, sim, R, n_cols + 3)
    mask = rng.integers(0, 1 << 32, size=(R, n_words), dtype=np.uint64).astype(np.uint32)
    live = np.array([1, 0, 1, 1, 0, 0, 1, 0, 1], dtype=np.uint8)
    got, _ = sim.run(vals, sim.BF16, mask, n_cols=n_cols, base_elems=1, live=live, mask_stride=n_words + 2)
    assert (got == sim.expected(vals, sim.BF16, mask, live, n_cols)).all()
    assert (got[live == 0] == vals[live == 0]).all()
    got, k = sim.run(vals, sim.BF16, mask, n_cols=n_cols, live=np.zeros(R, dtype=np.uint8))
    assert (got == vals).all() and sum(k) == 0
    got, k = sim.run(vals[:0], sim.BF16, mask[:0], n_cols=n_cols)
    assert got.shape == (0, n_cols + 3)


def test_self_check_under_host_sanitizers(tmp_path):
    """the simulation's own main(), a stand-alone program, built with AddressSanitizer and UBSan: the kernels' first half reads and writes
    nothing it should not"""
    import os
    import subprocess
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim", "maskapply_sim.cpp")
    exe = str(tmp_path / "maskapply_sim_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wno-unknown-pragmas", "-DMASKAPPLY_SIM_MAIN", "-o", exe, src])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "maskapply_sim: ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-1500:])
