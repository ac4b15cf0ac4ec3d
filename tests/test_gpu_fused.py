"""GPU tests (-m gpu) of the ONE-launch form of the tile-owned mode (csrc/spl_k_fuse.h; batches of up to 1536 tiles -- the bench headline,
Tokenizer.encode, most calls a user makes): every tile publishes its token count into one of two parity arrays, the tiles behind it poll
the counts for their base, the NEXT fused launch re-arms the other parity.  Every result is compared with the oracle (COracle.encode_packed),
ids and offsets, bit-exact, and every device call asserts the FORM it ran in from the per-kernel launch counts (include/splintr_hip.h,
spl_profile_read: slot 8, k_tile_out, stays 0 for a fused launch), so that a test meant for the fused path cannot quietly run the other one.

  1  tile counts either side of the 16-bit limit: a count of 65 534 and more goes to the 32-bit side array (fuse_publish `big`,
     fuse_word's 0xFFFF branch) -- counts 65 532 .. 65 537, i. e. count + 1 = 0xFFFD .. 0x10002;
  2  launch sequences on one handle that re-arm both parities (fuse_rearm, tile 0's sweep beyond its grid), interleaved with two-launch
     calls and an empty batch, every batch different from the one before;
  3  the polling layout: four counts per 64-bit word, 256 tiles per load slot, copy tile % 16 -- every tile count around those edges;
  4  three handles in flight on three streams, more tiles than can be resident at once (what bench.py's `pipelined` leg times).
"""
import ctypes
import os
import random

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_parity import _force_tiles, tok

pytestmark = pytest.mark.gpu

NAME = "cl100k_base"
TILE = {0: 800, 5: 864}                 # bytes a tile owns: geometry A (batches up to 1.25 MB), geometry B (forced by 5)
ALIGN = 21600                           # 27 tiles of 800 bytes = 25 tiles of 864: a tile starts here in both geometries
FUSE_MAX_TILES = 1536
POISON = 0x5A5A5A5A


# ------------------------------------------------------------------------------------------------
# helpers: options, which form ran, device calls
# ------------------------------------------------------------------------------------------------
def _lib():
    from splintr_amd import _ffi
    return _ffi.lib()


def _opt(t, k, v):
    from splintr_amd import _ffi
    assert _lib().spl_set_option(t.handle, k.encode(), int(v)) == 0, _ffi.last_error()


def _profile(t, on):
    assert _lib().spl_profile_enable(t.handle, 1 if on else 0) == 0


def _launches(t, call):
    """(calls that launched k_pretok, calls that launched k_tile_out) of `call()` on a handle whose profiling is on."""
    import torch
    L = _lib()
    assert L.spl_profile_reset(t.handle) == 0
    call()
    torch.cuda.synchronize()
    ms, n = (ctypes.c_double * 16)(), (ctypes.c_uint64 * 16)()
    assert L.spl_profile_read(t.handle, ms, n) == 0
    return int(n[2]), int(n[8])


def _poison(b):
    """What an earlier call left in the batch's output buffers must not pass for this call's result."""
    b.ids.fill_(POISON)
    b.out_off.fill_(-1)


def _encode(t, b, form, special=False):
    """One device call on `b`, its form asserted -- "fused": ONE launch; "two": k_pretok + k_tile_out; "empty": a batch without a byte,
    which launches neither (the offsets are cleared by a memset; the profile records such a call in both slots) -- ; returns the CSR."""
    from splintr_amd.device import encode_device, result_csr
    _poison(b)
    n_pretok, n_out = _launches(t, lambda: encode_device(t, b, special))
    assert n_pretok == 1, n_pretok
    ran = "empty" if b.n_bytes == 0 else "fused" if n_out == 0 else "two"
    assert ran == form and n_out == (0 if form == "fused" else 1), f"expected the {form} form: k_tile_out ran in {n_out} call(s), {b.n_bytes} bytes"
    if form == "empty":
        assert not b.out_off.any().item()
    return result_csr(b)


def oracle_csr(orc, texts, special=False):
    """test_gpu_parity's oracle_csr on SIXTEEN threads: a thread per CPU of a large host only slows the pool down, and the giant
    documents -- one chunk each, one thread each -- are fifteen side by side."""
    bs = [t.encode("utf-8") for t in texts]
    off = np.zeros(len(bs) + 1, dtype=np.uint64)
    if bs:
        np.cumsum([len(b) for b in bs], out=off[1:])
    return orc.encode_packed(np.frombuffer(b"".join(bs), dtype=np.uint8), off, special, threads=16)


def _same(got, want, what):
    ids, off = got
    assert np.array_equal(off, want[1]), f"{what}: offsets differ, first at document {_first_diff(off, want[1])}"
    assert np.array_equal(ids, want[0]), f"{what}: ids differ, first at token {_first_diff(ids, want[0])} of {len(want[0])}"


def _first_diff(a, b):
    n = min(len(a), len(b))
    d = np.nonzero(a[:n] != b[:n])[0]
    return int(d[0]) if len(d) else n


def _dev():
    import torch
    return torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------------
# helpers: text cut to an exact number of tiles
# ------------------------------------------------------------------------------------------------
_blobs = {}


def _blob(gen, seed):
    """1.5 MB and more of one corpus generator, as bytes."""
    from splintr_amd import corpus
    key = (gen, seed)
    if key not in _blobs:
        n = {"c2": 1500, "c2_wide": 1500, "c3": 420}[gen]
        _blobs[key] = "".join(getattr(corpus, gen)(n, seed=seed)).encode("utf-8")
        assert len(_blobs[key]) > FUSE_MAX_TILES * 864 + 8192, (gen, len(_blobs[key]))
    return _blobs[key]


def _exact(blob, at, n_bytes, n_docs, rng):
    """`n_bytes` bytes of `blob` from about `at` on, as `n_docs` documents (cut at character boundaries: the byte count is exact)."""
    text = blob[at:at + n_bytes].decode("utf-8", "ignore")
    text += "x" * (n_bytes - len(text.encode("utf-8")))               # (what the cut took from a character at either end)
    cuts = sorted(rng.sample(range(1, len(text)), min(n_docs - 1, len(text) - 1))) if len(text) > 1 else []
    docs = [text[a:b] for a, b in zip([0] + cuts, cuts + [len(text)])]
    assert sum(len(d.encode("utf-8")) for d in docs) == n_bytes
    return docs


def _tiles(gen, seed, k, rng, tile=800, short=None):
    """Documents of exactly k tiles: (k - 1) * tile < bytes <= k * tile, the last tile `short` bytes short of full (default: random)."""
    blob = _blob(gen, seed)
    if short is None:
        short = rng.choice((0, tile - 1, rng.randrange(tile)))
    n = k * tile - short
    assert (n + tile - 1) // tile == k
    return _exact(blob, rng.randrange(0, len(blob) - n - 4), n, 4 + k // 64, rng)


# ------------------------------------------------------------------------------------------------
# the giant documents: ONE chunk that no vocabulary entry shortens much, all of whose tokens belong to the tile it starts in
# ------------------------------------------------------------------------------------------------
GIANT_BASE = 65530
GIANT_M = (2, 3, 4, 5, 6, 7)            # the document of m has GIANT_BASE + m tokens: 65 532 .. 65 537
_giants = {}


def _letters():
    rng = random.Random(3)
    return "".join(rng.choice("qxzjkvwQXZJKVW") for _ in range(82000))


def _giant_doc(m, L, s):
    return "a" + " a" * (m - 1) + " " + s[:L]


def _per_doc(orc, docs):
    """The oracle's ids of each document, from ONE call (the pool encodes the documents side by side)."""
    ids, off = oracle_csr(orc, docs)
    return [ids[int(off[i]):int(off[i + 1])] for i in range(len(docs))]


def _token_bytes():
    """bytes of every cl100k token, by rank"""
    from oracle import pyoracle
    enc, _ = pyoracle.load_splv(os.path.join(ROOT, "splintr_amd", "data", NAME + ".splv"))
    n = np.zeros(max(enc.values()) + 1, dtype=np.int64)
    n[list(enc.values())] = [len(k) for k in enc]
    return n


def giants(coracle):
    """({m: document}, {document: the oracle's ids}), computed once per session.
    A run of random letters of "qxzjkvwQXZJKVW" behind a blank is ONE chunk that hardly merges; L is the first length at which it has
    65 530 tokens, and "a" + " a" * (m - 1) in front of it adds m tokens, all of them the tile's the document starts in.
    The oracle takes about 4 s per such document (the merge of one 80 KB chunk), so there are two calls only: the whole run, which says
    where its 65 530th token ends (L0; a PREFIX cut there or a letter earlier may end in other tokens than the run does), then -- side by
    side on the pool's threads -- the bare prefixes of L0 - 2 .. L0 letters, which say which of L0 - 1 and L0 is the first length, and
    the documents for both."""
    if _giants:
        return _giants["docs"], _giants["ids"]
    orc = coracle(NAME)
    s = _letters()
    whole = _per_doc(orc, [" " + s])[0]
    assert len(whole) > GIANT_BASE + 100
    L0 = int(np.cumsum(_token_bytes()[whole.astype(np.int64)])[GIANT_BASE - 1]) - 1
    docs = [" " + s[:L] for L in (L0 - 2, L0 - 1, L0)] + [_giant_doc(m, L, s) for L in (L0 - 1, L0) for m in GIANT_M]
    ids = dict(zip(docs, _per_doc(orc, docs)))
    count = {L: len(ids[" " + s[:L]]) for L in (L0 - 2, L0 - 1, L0)}
    first = [L for L in (L0 - 1, L0) if count[L - 1] < GIANT_BASE <= count[L]]
    assert len(first) == 1 and count[first[0]] == GIANT_BASE, (L0, count)
    out = {m: _giant_doc(m, first[0], s) for m in GIANT_M}
    for m, d in out.items():
        assert len(ids[d]) == GIANT_BASE + m, (m, len(ids[d]))              # the tile's count, from the oracle
        assert 2 * m < 800 and len(d.encode()) > 864                          # every token starts in the document's first tile, which holds no other document
    _giants["docs"], _giants["ids"] = out, {d: ids[d] for d in out.values()}
    return _giants["docs"], _giants["ids"]


def _want(coracle, texts, special=False, name=NAME):
    """The oracle's CSR of `texts`: the giants' ids from the session's one computation (they hold no special-token literal: the same ids
    with and without SPL_WITH_SPECIAL), the rest by one call."""
    known = _giants.get("ids", {}) if name == NAME else {}
    assert not any("<|" in t for t in known)
    rest = [t for t in texts if t not in known]
    r_ids, r_off = oracle_csr(coracle(name), rest, special)
    parts, k = [], 0
    for t in texts:
        if t in known:
            parts.append(known[t])
        else:
            parts.append(r_ids[int(r_off[k]):int(r_off[k + 1])])
            k += 1
    off = np.zeros(len(texts) + 1, dtype=np.uint64)
    if texts:
        np.cumsum([len(p) for p in parts], out=off[1:])
    ids = np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, dtype=np.uint32)
    return ids, off


def _pad_to(docs, n_bytes):
    """`docs` plus a filler document so that they take exactly n_bytes."""
    have = sum(len(d.encode("utf-8")) for d in docs)
    assert have < n_bytes
    return docs + [("pad to the tile edge, " * (n_bytes // 22 + 1))[:n_bytes - have]]


def _front(literal=""):
    """C2 text (with `literal` inside two of its documents) that ends on a tile edge of both geometries."""
    from splintr_amd import corpus
    docs, n = [], 0
    for i, d in enumerate(corpus.c2(40, seed=91)):
        if i in (1, 3):
            d = d[:len(d) // 3] + literal + d[len(d) // 3:]
        if n + len(d.encode("utf-8")) > ALIGN - 64:
            break
        docs.append(d)
        n += len(d.encode("utf-8"))
    assert len(docs) >= 4
    return _pad_to(docs, ALIGN)


def _after(seed=92, n=8):
    from splintr_amd import corpus
    return corpus.c2(n, seed=seed) + ["", "x"]


def _scenario(which, m, G):
    """The documents of one scenario around the giant document of m; every giant document starts on a tile edge of both geometries."""
    from splintr_amd import corpus
    g = G[m]
    if which == "tile0":                    # the giant tile is tile 0; every other tile reads its count
        docs = [g] + _after(93, 4)
    elif which == "inner":                  # the giant tile at index 27 (geometry B: 25), ordinary tiles in front of it
        docs = _front() + [g, "z"]
    elif which == "followed":               # ordinary documents behind it: a wrong base moves their ids and offsets
        docs = _front() + [g] + _after(94, 12) + corpus.c2(6, seed=95)
    elif which == "last":                   # the giant document last: only the (empty) tiles of its own text are behind its tile
        docs = _pad_to(_after(96, 6), ALIGN) + [g]
    else:                                   # two giant tiles in one batch, counts on both sides of the limit (m and 9 - m)
        assert which == "two"
        head = _front() + [g]
        n = sum(len(d.encode("utf-8")) for d in head)
        docs = _pad_to(head + corpus.c2(4, seed=97), (n // ALIGN + 2) * ALIGN) + [G[9 - m]] + _after(98, 5)
    at, pos = [], 0
    for d in docs:
        if d in (g, G[9 - m]):
            at.append(pos)
        pos += len(d.encode("utf-8"))
    assert at and all(a % ALIGN == 0 for a in at), at                  # a giant document starts its tile: the tile's count IS the document's
    assert pos <= 1200 * 800
    return docs


# ------------------------------------------------------------------------------------------------
# 1  tile counts either side of the 16-bit limit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", [0, 5])
@pytest.mark.parametrize("which", ["tile0", "inner", "followed", "last", "two"])
def test_tile_counts_around_the_16_bit_limit(coracle, which, geom):
    """A tile of 65 532 .. 65 537 tokens (count + 1 = 0xFFFD .. 0x10002: the 16-bit word up to 0xFFFE, from 65 534 tokens on 0xFFFF and the
    32-bit side word) at tile 0, behind ordinary tiles, in front of ordinary documents, as the last document, and twice in one batch: as ONE
    launch and as two, both the oracle's CSR; one call through the host path (spl_encode_batch) per scenario."""
    from splintr_amd.device import DeviceBatch
    G, _ = giants(coracle)
    t = tok(NAME)
    _force_tiles(NAME, geom)
    _profile(t, True)
    try:
        for m in GIANT_M:
            docs = _scenario(which, m, G)
            want = _want(coracle, docs)
            b = DeviceBatch(docs, _dev())
            for fuse in (1, 0):
                _opt(t, "fuse", fuse)
                _same(_encode(t, b, "fused" if fuse else "two"), want, f"{which} {GIANT_BASE + m} tokens, geometry {geom}, fuse {fuse}")
            if m == 4 + geom // 5:              # (65 534 tokens: the first count of the side array; 65 535 in geometry B)
                _same(t.encode_batch_csr(docs), want, f"{which} host path")
    finally:
        _opt(t, "fuse", 1)
        _profile(t, False)
        _force_tiles(NAME, 0)


@pytest.mark.parametrize("geom", [0, 5])
def test_a_giant_tile_with_special_tokens(coracle, geom):
    """SPL_WITH_SPECIAL (the literal scan in front of the one launch, the tiles skip the literals' spans): the giant tile in the middle,
    <|endoftext|> in the ordinary documents in front of and behind it."""
    from splintr_amd.device import DeviceBatch
    G, _ = giants(coracle)
    t = tok(NAME)
    front = _front("<|endoftext|>")
    docs = front + [G[5]] + [d[:40] + "<|endoftext|><|endoftext|>" + d[40:] for d in _after(94, 12)]
    want = _want(coracle, docs, special=True)
    at = len(front)
    assert int(want[1][at + 1] - want[1][at]) == GIANT_BASE + 5               # the giant tile's count, from the oracle
    assert int(np.count_nonzero(want[0] == 100257)) == 2 + 2 * 14           # <|endoftext|> as ONE id, in front of and behind it
    b = DeviceBatch(docs, _dev())
    _force_tiles(NAME, geom)
    _profile(t, True)
    try:
        for fuse in (1, 0):
            _opt(t, "fuse", fuse)
            _same(_encode(t, b, "fused" if fuse else "two", special=True), want, f"special, geometry {geom}, fuse {fuse}")
        _same(t.encode_batch_csr(docs, with_special=True), want, "special, host path")
    finally:
        _opt(t, "fuse", 1)
        _profile(t, False)
        _force_tiles(NAME, 0)


@pytest.mark.parametrize("geom", [0, 5])
@pytest.mark.parametrize("m", [4, 6])
def test_a_giant_tile_into_a_slab(coracle, geom, m):
    """spl_encode_batch_device_packed: the fused launch writes the all-gather slab too -- header, offsets and ids take the same base -- and
    must leave what encode + spl_gatherv_pack leave (as test_encode_packed_slab_equals_pack_kernel compares them), and the oracle's CSR."""
    import torch
    from splintr_amd.device import DeviceBatch, result_csr
    G, _ = giants(coracle)
    t = tok(NAME)
    L = _lib()
    dev = _dev()
    stream = torch.cuda.current_stream(dev).cuda_stream
    docs = _scenario("followed", m, G)
    want = _want(coracle, docs)
    bt = DeviceBatch(docs, dev)
    _force_tiles(NAME, geom)
    _profile(t, True)
    try:
        _same(_encode(t, bt, "fused"), want, "encode")
        T = int(want[1][-1])
        max_docs, cap = bt.n_docs + 3, T + bt.n_docs + 3 + 4 + 11
        ref = torch.zeros(cap, dtype=torch.int32, device=dev)
        assert L.spl_gatherv_pack(t.handle, bt.ids.data_ptr(), bt.out_off.data_ptr(), bt.n_docs, ref.data_ptr(), cap, max_docs, stream) == 0
        got = torch.zeros(cap, dtype=torch.int32, device=dev)
        b2 = DeviceBatch(docs, dev)
        _poison(b2)
        n_pretok, n_out = _launches(t, lambda: L.spl_encode_batch_device_packed(
            t.handle, b2.text.data_ptr(), b2.n_bytes, b2.doc_off.data_ptr(), b2.n_docs, 0, b2.ids.data_ptr(), b2.ids.numel(),
            b2.out_off.data_ptr(), got.data_ptr(), cap, max_docs, stream))
        assert (n_pretok, n_out) == (1, 0)                               # ONE launch
    finally:
        _profile(t, False)
        _force_tiles(NAME, 0)
    _same(result_csr(b2), want, "encode into a slab")
    used = 3 + max_docs + T
    r, g = ref[:used].cpu().numpy(), got[:used].cpu().numpy()
    assert int(g[0]) == T and int(g[1]) == bt.n_docs
    assert np.array_equal(r[: 2 + bt.n_docs + 1], g[: 2 + bt.n_docs + 1])          # (offsets beyond n_docs + 1: unspecified padding in both)
    assert np.array_equal(r[3 + max_docs:], g[3 + max_docs:])
    assert np.array_equal(g[3 + max_docs:].view(np.uint32), want[0])


# ------------------------------------------------------------------------------------------------
# 2  launch sequences that re-arm both parities
# ------------------------------------------------------------------------------------------------
def test_a_sequence_of_different_batches_re_arms_both_parities(coracle):
    """Launch N publishes into parity N % 2 and zeroes what launch N - 1 left in the other one: each tile its own entries (sixteen copies of
    the 16-bit count by lanes 0 .. 15, the 32-bit side word by lane 16), tile 0 the entries beyond this launch's grid.  A count that
    survives is read by launch N + 1 as a tile's count -- it never waits for a non-zero word.  One handle, a fixed sequence in which no
    batch equals the one before it (replaying a batch would make a stale count the right one), every result against the oracle.
    What this can and cannot show: a stale 16-BIT count gives wrong bases in the next launch on its parity, and the sequence has such a
    launch behind every sweep and every re-arm.  A stale SIDE word is read only behind a 16-bit 0xFFFF (fuse_word), and the tile that
    stores the 0xFFFF has stored its new side word one instruction earlier from the same lane (fuse_publish): it shows only if a reader
    sees those two stores out of order.  The steps with a giant tile at the index of an earlier one (another count each time) are where
    that would show; without such a reordering the two side-word stores of the re-arm are not observable from results."""
    from splintr_amd import Tokenizer
    from splintr_amd.device import DeviceBatch, reserve
    G, _ = giants(coracle)
    rng = random.Random(1234)
    t = Tokenizer.from_pretrained(NAME)
    _profile(t, True)
    dev = _dev()

    def giant_batch(m, seed):               # eight ordinary tiles, the giant tile (index 8), ordinary documents behind it
        return _tiles("c2", 61, 8, rng, short=0) + [G[m]] + _after(seed, 10)

    first = giant_batch(6, 71)              # 65 536 tokens in tile 8: the side word
    big_a, big_b = _tiles("c3", 62, FUSE_MAX_TILES, rng), _tiles("c2_wide", 63, FUSE_MAX_TILES, rng)
    steps = [                               # (what, documents, form, options around the call)
        ("a giant tile at index 8", first, "fused", {}),
        ("3 tiles: the giant's entries lie beyond this grid, they are tile 0's sweep's", _tiles("c3", 62, 3, rng), "fused", {}),
        ("230 tiles on the parity the giant used", _tiles("c2_wide", 63, 230, rng), "fused", {}),
        ("1 tile", _tiles("c2", 61, 1, rng), "fused", {}),
        ("an empty batch", ["", ""], "empty", {}),
        ("1536 tiles", big_a, "fused", {}),
        ("300 tiles as two launches (fuse 0)", _tiles("c2", 64, 300, rng), "two", {"fuse": 0}),
        ("2 tiles", _tiles("c2_wide", 63, 2, rng), "fused", {}),
        ("1536 tiles of other text", big_b, "fused", {}),
        ("1537 tiles: two launches", _tiles("c3", 65, FUSE_MAX_TILES + 1, rng), "two", {}),
        ("4 tiles with fuse_max_tiles 4", _tiles("c3", 62, 4, rng), "fused", {"fuse_max_tiles": 4}),
        ("5 tiles with fuse_max_tiles 4", _tiles("c2", 64, 5, rng), "two", {"fuse_max_tiles": 4}),
        ("a giant tile at index 8 again, 65 534 tokens", giant_batch(4, 72), "fused", {}),
        ("400 tiles: the giant's index exists in this grid, its entries are the re-arm's (fuse_rearm), not the sweep's", _tiles("c3", 65, 400, rng), "fused", {}),
        ("150 tiles", _tiles("c2_wide", 66, 150, rng), "fused", {}),
        ("7 tiles", _tiles("c2", 64, 7, rng), "fused", {}),
        ("a giant tile at index 8 on the parity of the last one, 65 537 tokens", giant_batch(7, 73), "fused", {}),
        ("90 tiles", _tiles("c3", 62, 90, rng), "fused", {}),
        ("the first batch again", first, "fused", {}),
    ]
    default = {"fuse": 1, "fuse_max_tiles": FUSE_MAX_TILES}
    # the workspace for the largest batch first: a handle that GROWS allocates its count arrays anew, all zero, and would hide what the
    # launch before left in them
    reserve(t, max(sum(len(d.encode("utf-8")) for d in s[1]) for s in steps), max(len(s[1]) for s in steps))
    for i, (what, docs, form, opts) in enumerate(steps):
        if i:
            assert docs != steps[i - 1][1]
        want = _want(coracle, docs)
        b = DeviceBatch(docs, dev)
        for k, v in opts.items():
            _opt(t, k, v)
        try:
            _same(_encode(t, b, form), want, f"step {i}: {what}")
        finally:
            for k in opts:
                _opt(t, k, default[k])
    # the host path on the same handle (its chunks are launches of the handle's first context too), behind the sequence so that the parities
    # above do not depend on the form its calls take; then a device call again
    for what, docs in (("the first batch", first), ("90 tiles", steps[-2][1])):
        _same(t.encode_batch_csr(docs), _want(coracle, docs), f"host path: {what}")
    docs = _tiles("c2", 64, 150, rng)
    _same(_encode(t, DeviceBatch(docs, dev), "fused"), _want(coracle, docs), "150 tiles behind the host calls")


# ------------------------------------------------------------------------------------------------
# 3  polling layout
# ------------------------------------------------------------------------------------------------
K_ALL = (list(range(1, 10)) + list(range(15, 19)) + list(range(31, 35)) + list(range(63, 67)) + list(range(255, 259)) +
         list(range(511, 515)) + list(range(767, 771)) + list(range(1023, 1027)) + list(range(1279, 1283)) + list(range(1533, 1538)))
K_GEOM_B = [k for k in K_ALL if k <= 258 or k >= 1533]


@pytest.mark.parametrize("geom", [0, 5])
@pytest.mark.parametrize("name", ["cl100k_base", "o200k_base"])
def test_every_tile_count_around_the_edges_of_the_polling_layout(coracle, name, geom):
    """A tile reads the counts in front of it four to a 64-bit word, one word per lane and load slot (256 tiles a slot, six slots), from copy
    tile % 16 of the array: batches of exactly k tiles of the C3 mix (several documents each), k around every such edge up to 1536 -- the
    largest fused launch -- and 1537, which must take two launches.  (19 MB of ordinary text in all: half a second of the oracle.)"""
    from splintr_amd.device import DeviceBatch, reserve
    rng = random.Random(300 + geom)
    t = tok(name)
    batches = [(k, _tiles("c3", 77, k, rng, tile=TILE[geom])) for k in (K_ALL if geom == 0 else K_GEOM_B)]
    # ONE oracle call for all of them
    flat = [d for _, docs in batches for d in docs]
    ids, off = oracle_csr(coracle(name), flat)
    # (the workspace for the largest batch first: a handle that grows allocates its count arrays anew, all zero -- with it every batch
    #  here finds the counts of the batch before it, of another size, in the parity it re-arms)
    reserve(t, max(sum(len(d.encode("utf-8")) for d in docs) for _, docs in batches), max(len(docs) for _, docs in batches))
    _force_tiles(name, geom)
    _profile(t, True)
    try:
        at = 0
        for k, docs in batches:
            lo, hi = int(off[at]), int(off[at + len(docs)])
            want = (ids[lo:hi], off[at:at + len(docs) + 1] - off[at])
            at += len(docs)
            b = DeviceBatch(docs, _dev())
            _same(_encode(t, b, "fused" if k <= FUSE_MAX_TILES else "two"), want, f"{name}: {k} tiles of {TILE[geom]} bytes")
    finally:
        _profile(t, False)
        _force_tiles(name, 0)


# ------------------------------------------------------------------------------------------------
# 4  three handles in flight
# ------------------------------------------------------------------------------------------------
def test_three_handles_in_flight_on_three_streams(coracle):
    """Three fused launches on three streams hold more tiles (1800) than can be resident (1536); a tile only waits for tiles of ITS launch
    with a lower index, which were dispatched before it.  Six rounds round-robin without a synchronisation in between, another set of
    batches from the fourth round on; one synchronisation, then all six results against the oracle."""
    import torch
    from splintr_amd import Tokenizer
    from splintr_amd.device import DeviceBatch, encode_device, pick_stream, reserve, result_csr
    dev = _dev()
    rng = random.Random(4321)
    sets = [[_tiles("c2", 81, 600, rng), _tiles("c2_wide", 82, 605, rng), _tiles("c3", 83, 595, rng)],
            [_tiles("c2", 84, 590, rng), _tiles("c2_wide", 85, 612, rng), _tiles("c3", 86, 598, rng)]]
    wants = [[_want(coracle, docs) for docs in s] for s in sets]
    batches = [[DeviceBatch(docs, dev) for docs in s] for s in sets]
    toks = [Tokenizer.from_pretrained(NAME) for _ in range(3)]
    streams = [torch.cuda.current_stream(dev)]
    while len(streams) < 3:
        streams.append(pick_stream(dev, streams))
    # the form, asserted where asserting it may synchronise: each handle's first call on each of its batches
    for h, t in enumerate(toks):
        reserve(t, max(s[h].n_bytes for s in batches), max(s[h].n_docs for s in batches))
        _profile(t, True)
        for s in (0, 1):
            _same(_encode(t, batches[s][h], "fused"), wants[s][h], f"handle {h}, set {s}, alone")
        _profile(t, False)
    for s in batches:
        for b in s:
            _poison(b)
    torch.cuda.synchronize()
    for rnd in range(6):
        for h, t in enumerate(toks):
            with torch.cuda.stream(streams[h]):
                encode_device(t, batches[rnd // 3][h])
    torch.cuda.synchronize()
    for s in (0, 1):
        for h in range(3):
            _same(result_csr(batches[s][h]), wants[s][h], f"handle {h}, set {s}, three in flight")
