"""GPU tests (-m gpu) of what spl_encode_batch_device promises about the CALLER'S buffers (include/splintr_hip.h, next to the call):

  capacity   tokens beyond ids_capacity are dropped, d_out_off is complete whatever the capacity is (d_out_off[n_docs] is the need);
  footprint  nothing is stored at or beyond d_ids[T], in front of d_ids[0] or outside d_out_off[0 .. n_docs];
  text tail  the bytes behind d_utf8[n_bytes] are the caller's: the result is that of the n_bytes bytes alone.

Every call goes through the C ABI with ctypes.  d_ids is a view of exactly `cap` entries and d_out_off one of n_docs + 1 entries, each INSIDE
an allocation with guard elements in front and behind, all of it a sentinel (test_gpu_collate.Guarded; 0x5A5A5A5A is above 2^21, never an
id): after the call the offsets are the oracle's in full, ids[:min(cap, T)] is the oracle's prefix, ids[T:cap] still holds the sentinel,
and the four guards are intact.  The text is one allocation: the corpus from a 16-byte boundary on, then a tail of at least 80 bytes that
is NOT zero.  Expected values: the C oracle (COracle.encode_packed) on exactly the n_bytes bytes -- for the custom-pattern handle the
Python oracle with the same pattern string --, bit-exact.  Every call asserts the form it ran in from the per-kernel launch counts
(spl_profile_read: slot 6, k_range_count, runs in queue mode only; slot 8, k_tile_out, stays 0 for the one fused launch).

  A  capacities below, at and above the token count, in all four forms (fused, two launches, geometry 5, queue mode);
  B  capacities inside the tokens that START beyond a tile's window (stage[]: the second loop of k_tile_out, the matching loop of the
     fused path, k_range_out's third source);
  C  the other entry points: SPL_WITH_SPECIAL (fast scan and general matcher), a custom split pattern (with and without the patched
     second tile pass), given boundaries (spl_encode_chunks_device), the slab form (spl_encode_batch_device_packed, both slab formats);
  D  the result does not depend on the bytes behind n_bytes: endings that a continuation would change, at every n_bytes % 16.
"""
import contextlib
import ctypes
import json
import os
import random

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_collate import SENT, Guarded, _dev
from test_gpu_fused import _launches, _opt, _profile
from test_gpu_parity import _force_tiles, tok
from test_host_regex import GPT2_PATTERN

pytestmark = pytest.mark.gpu

VOCABS2 = ("cl100k_base", "o200k_base")
FORMS = {"fused": (0, 1), "two": (0, 0), "geom5": (5, 1), "queue": (4, 1)}      # form -> (forced mode, option "fuse")
RAN = {"fused": "fused", "two": "two", "geom5": "fused", "queue": "queue"}       # ... and what the launch counts then show
SPECIAL = 1                                                                      # SPL_WITH_SPECIAL
EOT = "<|endoftext|>"
TAIL = (b"ing's 123  \n\nand on " * 8)[:96]         # behind n_bytes by default: text that would continue a word, a number, a blank run
SLAB_FILL = 0xA5A5A5A5                              # the slab's own pre-fill: differs from the sentinel in d_ids
DATA = os.path.join(ROOT, "splintr_amd", "data")


# ------------------------------------------------------------------------------------------------
# helpers: the library, forms, a corpus on the device
# ------------------------------------------------------------------------------------------------
def _lib():
    from splintr_amd import _ffi
    return _ffi.lib()


def _stream():
    import torch
    return torch.cuda.current_stream(_dev()).cuda_stream


@contextlib.contextmanager
def _form(name, form):
    """tok(name) forced into `form`, its profiling on; everything is put back whatever happens.  A forced mode this build does not know
    (spl_debug_phases refuses it) skips the parameter."""
    t = tok(name)
    mode, fuse = FORMS[form]
    st = (ctypes.c_uint64 * 16)()
    if _lib().spl_debug_phases(t.handle, mode << 1, st) != 0:
        _force_tiles(name, 0)
        pytest.skip(f"forced mode {mode} is not compiled in")
    try:
        _force_tiles(name, mode)
        _opt(t, "fuse", fuse)
        _profile(t, True)
        yield t
    finally:
        _opt(t, "fuse", 1)
        _profile(t, False)
        _force_tiles(name, 0)


def _ran(t, call):
    """the form `call()` ran in on a handle whose profiling is on: "queue", "fused" (ONE launch) or "two" (k_pretok + k_tile_out)"""
    n_pretok, n_out = _launches(t, call)
    ms, n = (ctypes.c_double * 16)(), (ctypes.c_uint64 * 16)()
    assert _lib().spl_profile_read(t.handle, ms, n) == 0
    assert n_pretok == 1, n_pretok
    return "queue" if n[6] else "fused" if n_out == 0 else "two"


class Corpus:
    """Documents (bytes) packed into ONE uint8 allocation on the device: the corpus from a 16-byte boundary on, `tail` right behind
    n_bytes (at least 80 bytes of the caller's choosing), then zeros up to a multiple of 16."""

    def __init__(self, docs, tail=TAIL):
        import torch
        docs = [d.encode("utf-8") if isinstance(d, str) else d for d in docs]
        self.docs = docs
        self.blob = b"".join(docs)
        self.n_bytes, self.n_docs = len(self.blob), len(docs)
        self.off = np.zeros(self.n_docs + 1, dtype=np.uint64)
        np.cumsum([len(d) for d in docs], out=self.off[1:])
        assert len(tail) >= 80
        host = self.blob + tail
        host += b"\0" * ((-len(host)) % 16)
        self.text = torch.from_numpy(np.frombuffer(host, dtype=np.uint8).copy()).to(_dev())
        assert self.text.data_ptr() % 16 == 0
        self.d_off = torch.from_numpy(self.off.astype(np.int64)).to(_dev())

    def want(self, orc, special=False):
        """the C oracle's CSR of exactly the n_bytes bytes"""
        return orc.encode_packed(np.frombuffer(self.blob, dtype=np.uint8), self.off, special, threads=8)


class Slab:
    """An ample all-gather slab in a guarded buffer of its own, pre-filled with SLAB_FILL."""

    def __init__(self, T, n_docs, pack24):
        import torch
        from splintr_amd.device import _slab_words
        self.pack24, self.n_docs, self.max_docs = pack24, n_docs, n_docs + 3
        self.cap_words = _slab_words(T + 11, self.max_docs, pack24)
        self.g = Guarded(self.cap_words, torch.int32)
        self.g.view.fill_(SLAB_FILL - (1 << 32))
        self.fill = SLAB_FILL & 0xFFFFFF if pack24 else SLAB_FILL

    def read(self, n):
        """(T, N, offsets[n_docs + 1], the ids at ranks 0 .. n - 1) as they lie in the slab; the slab's guards are checked"""
        w = self.g.host().view(np.uint32)
        area = w[3 + self.max_docs:]
        if self.pack24:
            b = area.view(np.uint8).astype(np.uint32)
            k = 3 * np.arange(n)
            ids = b[k] | (b[k + 1] << 8) | (b[k + 2] << 16)
        else:
            ids = area[:n].copy()
        return int(w[0]), int(w[1]), w[2:2 + self.n_docs + 1].copy(), ids


def _call(t, c, cap, want, what, *, flags=0, form=None, slab=None, bits=None):
    """ONE device encode of corpus `c` into guarded buffers of exactly `cap` ids and n_docs + 1 offsets, everything the header promises
    asserted against want = (ids, offsets).  form: what the launch counts must show (None: a handle without profiling, not asserted);
    slab: through spl_encode_batch_device_packed; bits: through spl_encode_chunks_device with these two device bitmaps.
    Returns (ids[cap], offsets) as the call left them."""
    import torch
    from splintr_amd import _ffi
    L = _lib()
    ids, out = Guarded(cap, torch.int32), Guarded(c.n_docs + 1, torch.int64)
    head = (t.handle, c.text.data_ptr(), c.n_bytes, c.d_off.data_ptr(), c.n_docs)
    if bits is not None:
        fn = lambda: L.spl_encode_chunks_device(*head, bits[0].data_ptr(), bits[1].data_ptr(), ids.ptr(), cap, out.ptr(), _stream())
    elif slab is not None:
        fn = lambda: L.spl_encode_batch_device_packed(*head, flags, ids.ptr(), cap, out.ptr(), slab.g.ptr(), slab.cap_words, slab.max_docs, _stream())
    else:
        fn = lambda: L.spl_encode_batch_device(*head, flags, ids.ptr(), cap, out.ptr(), _stream())
    rc = []
    if form is None:
        rc.append(fn())
        torch.cuda.synchronize()
    else:
        ran = _ran(t, lambda: rc.append(fn()))
    assert rc == [0], (what, _ffi.last_error())
    if form is not None:
        assert ran == form, f"{what}: expected the {form} form, the launch counts show {ran}"
    try:
        got_ids, got_off = ids.host().view(np.uint32), out.host()                 # (the four guards)
    except AssertionError as e:
        raise AssertionError(f"{what}, capacity {cap}: {e}") from e
    w_ids, w_off = want
    T = int(w_off[-1])
    assert np.array_equal(got_off.astype(np.uint64), w_off), f"{what}, capacity {cap}: the offsets are not the oracle's (T = {T}, got {int(got_off[-1])})"
    n = min(cap, T)
    assert np.array_equal(got_ids[:n], w_ids[:n]), f"{what}, capacity {cap}: ids differ, first at rank {int(np.nonzero(got_ids[:n] != w_ids[:n])[0][0])} of {T}"
    if cap > T:
        bad = np.nonzero(got_ids[T:] != SENT["int32"])[0]
        assert not len(bad), f"{what}, capacity {cap}: written at rank {T + int(bad[0])}, at or beyond the token count {T}"
    return got_ids, got_off


_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ------------------------------------------------------------------------------------------------
# the batches
# ------------------------------------------------------------------------------------------------
def _docs_a():
    """About 8 KB of corpus.c2 text -- ten tiles -- as twelve documents: an empty one at the front, one in the middle, two at the end
    (their offsets equal n_bytes)."""
    from splintr_amd import corpus
    text = "".join(corpus.c2(12, seed=401)).encode("utf-8")[:7900].decode("utf-8", "ignore")
    rng = random.Random(402)
    cuts = sorted(rng.sample(range(300, len(text) - 300), 7))
    parts = [text[a:b] for a, b in zip([0] + cuts, cuts + [len(text)])]
    docs = [""] + parts[:4] + [""] + parts[4:] + ["", ""]
    n = sum(len(d.encode("utf-8")) for d in docs)
    assert len(docs) == 12 and 9 * 800 < n <= 10 * 800 and 9 * 864 < n + 864
    return docs


def _corpus_a():
    return _cached("a", lambda: Corpus(_docs_a()))


def _caps_c(T):
    return [1, 257, T // 2, T - 1, T]


def _docs_special():
    """batch A with <|endoftext|> inside four documents, one of them at the very end of the corpus (the last two documents are empty)"""
    docs = _docs_a()
    docs[1] = docs[1][:len(docs[1]) // 3] + EOT + docs[1][len(docs[1]) // 3:]
    docs[3] = EOT + docs[3]
    docs[7] = docs[7][:len(docs[7]) // 2] + EOT + EOT + docs[7][len(docs[7]) // 2:]
    docs[9] = docs[9] + EOT
    assert "".join(docs).endswith(EOT) and docs[10] == docs[11] == ""
    return docs


def _docs_b():
    """test_gpu_parity.test_chunk_that_straddles_the_window_end's documents of (240, "Ⅷ"), all k in ONE batch"""
    pad = lambda n: ("lorem ipsum " * 400)[:n]
    return [pad(k) + "Ⅷ" + "0" * 240 + "ⅧⅧ" + " and the end" for k in range(0, 1000)]


def _vocab_blob(name):
    with open(os.path.join(DATA, name + ".splv"), "rb") as f:
        return f.read()


# ------------------------------------------------------------------------------------------------
# the custom-pattern handle and its oracle
# ------------------------------------------------------------------------------------------------
def _custom():
    """(a handle over cl100k_base with GPT2_PATTERN, the Python oracle with the same pattern string): the split by PCRE2 where the
    library is there, by Python's `regex` otherwise"""
    def make():
        from splintr_amd import Tokenizer
        from oracle import pyoracle as O
        enc, _ = O.load_splv(os.path.join(DATA, "cl100k_base.splv"))
        return Tokenizer.from_bytes(_vocab_blob("cl100k_base"), GPT2_PATTERN), O.Oracle(enc, GPT2_PATTERN, False, {}, "pcre2" if O.pcre2_available() else "regex")
    return _cached("custom", make)


def _host_bits(t, blob, off):
    """spl_split_host's two bitmaps of a packed HOST corpus of exactly len(blob) bytes"""
    from splintr_amd import _ffi
    words = len(blob) // 32 + 2
    st, gp = np.zeros(words, dtype=np.uint32), np.zeros(words, dtype=np.uint32)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    assert _lib().spl_split_host(t.handle, blob, off.ctypes.data, len(off) - 1, st.ctypes.data, gp.ctypes.data) == 0, _ffi.last_error()
    return st, gp


def _custom_want(coracle, c):
    """The CSR of corpus `c` under GPT2_PATTERN: every document split on its own bytes alone, every chunk merged by the Python oracle.
    A chunk of more than 128 bytes is merged by the C oracle instead (the Python merge is quadratic), after asserting that the C
    oracle's own pattern leaves it in one piece.  A document that is not valid UTF-8 (D's cut character) is no input for a regex
    engine: its chunks come from the host splitter, run on that document alone (tests/test_host_regex.py pins it to PCRE2)."""
    t, o = _custom()
    orc = coracle("cl100k_base")
    ids, off = [], [0]
    for d in c.docs:
        try:
            d.decode("utf-8")
            spans = o.split(d)
        except UnicodeDecodeError:
            st, gp = _host_bits(t, d, np.array([0, len(d)], dtype=np.uint64))
            assert not gp.any()
            starts = [p for p in range(len(d)) if (int(st[p >> 5]) >> (p & 31)) & 1]
            spans = list(zip(starts, starts[1:] + [len(d)]))
        assert [s for s, _ in spans] == [0] * bool(d) + [e for _, e in spans[:-1]] and (spans[-1][1] if spans else 0) == len(d)     # (the pattern tiles the text)
        for s, e in spans:
            chunk = d[s:e]
            if len(chunk) > 128:
                assert orc.split_bytes(chunk) == [0]
                ids += orc.encode_bytes(chunk)
            else:
                ids += o.encode_chunk(chunk)
        off.append(len(ids))
    return np.array(ids, dtype=np.uint32), np.array(off, dtype=np.uint64)


# ------------------------------------------------------------------------------------------------
# A  capacity below the need: plain text
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", VOCABS2)
def test_capacity_below_at_and_above_the_token_count(coracle, name, form):
    """Ten tiles, twelve documents; every capacity is distinct and the small ones land inside different tiles.  Capacity 0 is given a
    valid pointer.  With a capacity above T the ids behind rank T keep the sentinel."""
    c = _corpus_a()
    want = c.want(coracle(name))
    T = int(want[1][-1])
    assert T >= 600, T
    caps = [0, 1, 63, 64, 65, 255, 256, 257, T // 2, T - 1, T, T + 1, c.n_bytes]
    assert caps == sorted(set(caps)), caps
    with _form(name, form) as t:
        for cap in caps:
            _call(t, c, cap, want, f"{name}, {form}", form=RAN[form])


# ------------------------------------------------------------------------------------------------
# B  capacity inside the tokens that start beyond a window
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["fused", "two", "queue", "geom5"])
def test_capacity_inside_tokens_that_start_beyond_a_window(coracle, form):
    """A run of numbers (three to a chunk) closed by U+2167 outgrows its window at every alignment: the chain's last tokens start
    beyond the window and reach the CSR through stage[] -- the second loop of k_tile_out (the two-launch form), the matching loop of
    the fused launch, k_range_out's third source.  In queue mode spl_last_queue_counts shows that chains were deferred (their tokens
    come from stage[]); the tile-owned forms expose no record of it: there the batch is the one
    test_chunk_that_straddles_the_window_end pins that path with.  A third, a half, T - 1 and T; and, because a store that ignores the
    capacity shows only within a guard's width behind it, capacities 20 tokens in front of the end of documents whose run starts
    10 .. 60 bytes in front of a tile's end -- in each of the three geometries (tile + right halo = 992 bytes in all of them): 183 to
    233 bytes of the 246-byte run fit the window, the document's last tokens start beyond it."""
    name = "cl100k_base"
    c = _cached("b", lambda: Corpus(_docs_b()))
    want = _cached("b_want", lambda: c.want(coracle(name)))
    T = int(want[1][-1])
    in_runs = []
    for tile in (800, 864, 768):
        hit = [d for d in range(c.n_docs) if tile - 60 <= (int(c.off[d]) + d) % tile < tile - 10]       # (document d: d bytes of filler, then the run)
        assert len(hit) >= 3, (tile, hit)
        in_runs += [int(want[1][d + 1]) - 20 for d in (hit[0], hit[len(hit) // 2], hit[-1])]
    with _form(name, form) as t:
        for cap in [T // 3, T // 2, T - 1, T] + in_runs:
            _call(t, c, cap, want, f"{name}, {form}", form=RAN[form])
        if form == "queue":
            q = (ctypes.c_uint32 * 4)()
            assert _lib().spl_last_queue_counts(t.handle, q) == 0
            assert q[3] > 0, list(q)


# ------------------------------------------------------------------------------------------------
# C  the other entry points
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["two", "fused", "queue"])
@pytest.mark.parametrize("name", VOCABS2)
def test_capacity_with_special_tokens(coracle, name, form):
    """SPL_WITH_SPECIAL: <|endoftext|> in four documents, the last one ending the corpus (k_special_scan's p + len > n_bytes with a
    literal that ends exactly at n_bytes).  Queue mode has no form with special tokens (spl_mode.h): forced, the call runs tile-owned."""
    c = _cached("sp", lambda: Corpus(_docs_special()))
    want = c.want(coracle(name), special=True)
    with open(os.path.join(DATA, "special_tokens.json"), encoding="utf-8") as f:
        eot = json.load(f)[name][EOT]
    assert int(np.count_nonzero(want[0] == eot)) == 5 and int(want[0][-1]) == eot
    T = int(want[1][-1])
    with _form(name, form) as t:
        for cap in _caps_c(T):
            _call(t, c, cap, want, f"{name}, special, {form}", flags=SPECIAL, form="fused" if form == "queue" else RAN[form])


def test_capacity_with_the_general_special_matcher():
    """Literals that contain one another, chain, or are longer than the fast scan's 32 bytes (the set of
    test_special_token_sets_whose_occurrences_overlap) take k_special_ends / k_special_select; expected: the Python oracle."""
    from splintr_amd import Tokenizer, CL100K_BASE_PATTERN
    from oracle import pyoracle as O
    special = {"<|a|>": 100300, "<|a|>x": 100301, "a|><": 100302, "|>": 100303, "ab": 100304, "abc": 100305,
               "bcd": 100306, "aa": 100307, "aaa": 100308, "<|" + "long" * 20 + "|>": 100309, "\n\n": 100310, "é": 100311}
    t = Tokenizer.from_bytes(_vocab_blob("cl100k_base"), CL100K_BASE_PATTERN, special)
    enc, _ = O.load_splv(os.path.join(DATA, "cl100k_base.splv"))
    o = O.Oracle(enc, O.CL100K_BASE_PATTERN, False, special, engine="regex")
    rng = random.Random(403)
    atoms = list(special) + ["a", "b", "c", "d", "x", "<", "|", ">", " ", "\n", "hello ", "é", "世界", "<|a", "|>x", "aaaa", "abcd", "<|a|"]
    texts = ["".join(rng.choice(atoms) for _ in range(rng.randint(0, 40))) for _ in range(120)]
    texts += ["<|a|>x<|a|>", "abcd", "aaaaa", "<|a|><|a|>x|>", "a|><|a|>", "<|" + "long" * 20 + "|>!", "", "<|" + "long" * 20 + "|>"]
    per = [o.encode_with_special(s) for s in texts]
    want = (np.array([i for p in per for i in p], dtype=np.uint32), np.cumsum([0] + [len(p) for p in per]).astype(np.uint64))
    T = int(want[1][-1])
    assert T > 600 and int(want[0][-1]) == 100309
    _call(t, Corpus(texts), T // 2, want, "general matcher", flags=SPECIAL)


def _docs_run():
    """batch A with a 3 000-byte run of '=' inside one document: a match the device splitter gives up on"""
    docs = _docs_a()
    docs[3] = docs[3][:100] + " " + "=" * 3000 + " " + docs[3][100:]
    return docs


@pytest.mark.parametrize("run", [False, True])
def test_capacity_with_a_custom_pattern(coracle, run):
    """A handle with GPT2_PATTERN through spl_encode_batch_device: the device splitter in front of the tile kernel.  With a 3 000-byte
    run in one document the splitter gives up on that document, it is split on the host and the tile pass runs AGAIN on the patched
    bitmaps into the same buffers (spl_device_split_fallbacks rises by one per call): the first pass's ids must not survive anywhere,
    so this one is also run with a capacity above T."""
    t, _ = _custom()
    c = _cached(("custom", run), lambda: Corpus(_docs_run() if run else _docs_a()))
    want = _cached(("custom_want", run), lambda: _custom_want(coracle, c))
    T = int(want[1][-1])
    assert T >= 600
    for cap in _caps_c(T) + [T + 1, c.n_bytes]:
        before = _lib().spl_device_split_fallbacks(t.handle)
        _call(t, c, cap, want, "custom pattern" + (", patched second pass" if run else ""))
        assert _lib().spl_device_split_fallbacks(t.handle) - before == (1 if run else 0)


def test_capacity_with_given_boundaries(coracle):
    """spl_encode_chunks_device: the two bitmaps from spl_split_host, device copies of exactly n_bytes / 32 + 2 words"""
    import torch
    t, _ = _custom()
    c = _corpus_a()
    want = _cached(("custom_want", False), lambda: _custom_want(coracle, c))
    st, gp = _host_bits(t, c.blob, c.off)
    bits = [torch.from_numpy(x.view(np.int32)).to(_dev()) for x in (st, gp)]
    T = int(want[1][-1])
    for cap in _caps_c(T) + [c.n_bytes]:
        _call(t, c, cap, want, "given boundaries", bits=bits)


def _check_slab(slab, want, cap, what):
    w_ids, w_off = want
    T = int(w_off[-1])
    hT, hN, off, ids = slab.read(T + 8)
    assert (hT, hN) == (T, slab.n_docs), f"{what}, capacity {cap}: the slab's header says T {hT}, N {hN}"
    assert np.array_equal(off, w_off.astype(np.uint32)), f"{what}, capacity {cap}: the slab's offsets"
    n = min(cap, T)
    assert np.array_equal(ids[:n], w_ids[:n]), f"{what}, capacity {cap}: the slab's ids below the capacity"
    # at or beyond ids_capacity the slab is promised nothing of the encode: the right id (the tile-owned mode fills the slab from the
    # tiles' own ids) or what the caller had there -- never something read from behind d_ids[ids_capacity]
    bad = np.nonzero((ids[n:T] != w_ids[n:T]) & (ids[n:T] != slab.fill))[0]
    assert not len(bad), f"{what}, capacity {cap}: slab id at rank {n + int(bad[0])} is {int(ids[n + bad[0]]):#x}: neither the id nor the slab's pre-fill"
    assert (ids[T:] == slab.fill).all(), f"{what}, capacity {cap}: the slab was written behind its T ids"


@pytest.mark.parametrize("pack24", [False, True])
@pytest.mark.parametrize("form", ["fused", "two", "queue"])
@pytest.mark.parametrize("name", VOCABS2)
def test_capacity_in_the_slab_form(coracle, name, form, pack24):
    """spl_encode_batch_device_packed with an ample slab: header, offsets and the ids below the capacity are right in every form; in
    queue mode the slab is copied out of d_ids by a queued k_gatherv_pack, which must stop at ids_capacity (it copied min(T, slab
    capacity) ids: whatever lay behind the caller's d_ids -- here the guard's sentinel -- travelled in the slab)."""
    from splintr_amd.device import _set_pack24
    c = _corpus_a()
    want = c.want(coracle(name))
    T = int(want[1][-1])
    with _form(name, form) as t:
        try:
            _set_pack24(t, pack24)
            for cap in _caps_c(T):
                slab = Slab(T, c.n_docs, pack24)
                what = f"{name}, slab{' (24-bit ids)' if pack24 else ''}, {form}"
                _call(t, c, cap, want, what, form=RAN[form], slab=slab)
                _check_slab(slab, want, cap, what)
        finally:
            _set_pack24(t, False)


@pytest.mark.parametrize("pack24", [False, True])
@pytest.mark.parametrize("form", ["fused", "queue"])
def test_an_empty_batch_in_the_slab_form(coracle, form, pack24):
    """n_bytes 0 launches no tile in any mode: the offsets are cleared by a fill and the slab is written by the same queued pack launch"""
    from splintr_amd.device import _set_pack24
    name = "cl100k_base"
    c = Corpus(["", "", ""])
    want = c.want(coracle(name))
    assert c.n_bytes == 0 and not want[1].any() and len(want[0]) == 0
    with _form(name, form) as t:
        try:
            _set_pack24(t, pack24)
            for cap in (0, 4):
                slab = Slab(0, c.n_docs, pack24)
                _call(t, c, cap, want, f"empty batch, slab, {form}", form="two", slab=slab)      # (no tile: the profile counts the call in both slots)
                _check_slab(slab, want, cap, f"empty batch, slab, {form}")
        finally:
            _set_pack24(t, False)


# ------------------------------------------------------------------------------------------------
# D  the result does not depend on the bytes behind n_bytes
# ------------------------------------------------------------------------------------------------
# (how the corpus ends, the tail most likely to change the result, flags)
ENDINGS = [(b" hel", b"lo world", 0),
           (b" 12", b"345 ", 0),
           (b" a  ", b"b", 0),                       # \s+(?!\S) takes the whole run only at the end of the text
           (b" x\n", b"\n\ny", 0),
           (b" don", b"'t ", 0),
           (b"!", b"!!\n\n", 0),
           (b" A", b"bc", 0),                        # o200k's case runs
           (b" \xe4\xbd", b"\xa0" + b"\x80" * 95, 0),        # a cut character, and what would complete it
           (b" <|endof", b"text|>", SPECIAL)]
PLAIN_TAILS = (b"\x00", b"\xff", b" ")


def _tails(unit):
    return [unit if len(unit) >= 80 else (unit * 96)[:96]] + [u * 96 for u in PLAIN_TAILS]


def _docs_d(ending, r):
    """About 2 KB of c2 text in three documents, the last one ending in `ending`, behind 0..15 filler bytes so that n_bytes % 16 == r
    (at 0 the tail begins a fresh 16-byte piece)"""
    def base():
        from splintr_amd import corpus
        a, b, d = corpus.c2(3, seed=404)
        return [a[:700].encode("utf-8"), b[:650].encode("utf-8"), d[:610].rstrip().encode("utf-8") + b"w"]
    docs = list(_cached("d_base", base))
    docs[2] = docs[2] + ending
    fill = (r - sum(len(d) for d in docs)) % 16
    docs[0] = b"pad pad pad pad pad "[:fill] + docs[0]
    assert sum(len(d) for d in docs) % 16 == r
    return docs


def _sweep_tails(run):
    """run(ending, flags, r, corpus of one tail) -> (ids, offsets) for every ending, every n_bytes % 16 and every tail; the results of
    one ending and alignment must be identical across the tails"""
    for ending, unit, flags in ENDINGS:
        for r in range(16):
            docs = _docs_d(ending, r)
            first = None
            for tail in _tails(unit):
                got = run(ending, flags, r, Corpus(docs, tail))
                if first is None:
                    first = got
                assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1]), (ending, r, tail[:8])


@pytest.mark.parametrize("form", ["fused", "two", "queue"])
@pytest.mark.parametrize("name", ["cl100k_base", "o200k_base", "mistral_v3"])
def test_the_result_does_not_depend_on_the_bytes_behind_the_text(coracle, name, form):
    """The end of the corpus takes code of its own -- the byte-wise branch of text16, iB / iT (the first index past the text),
    last_tile, k_special_scan's p + len > n_bytes, mask_tail behind load32 -- that has only ever been followed by zeros.  Capacity
    n_bytes: ids[T:] must keep the sentinel too.
    (What this can show: without k_special_scan's bound the <|endof ending fails here.  text16's byte-wise branch is a second line of
    defence: with the plain 16-byte load in its place every case still passes, because every reader of the staged window stops at iB.)"""
    orc = coracle(name)
    with _form(name, form) as t:
        def run(ending, flags, r, c):
            ran = "fused" if (form == "queue" and flags) else RAN[form]           # (no queue mode with special tokens)
            return _call(t, c, c.n_bytes, c.want(orc, bool(flags)), f"{name}, {form}, ending {ending!r}, n_bytes % 16 = {r}", flags=flags, form=ran)
        _sweep_tails(run)


def test_the_custom_pattern_s_result_does_not_depend_on_the_bytes_behind_the_text(coracle):
    """The same through the device splitter (its own bounds: a look-ahead or a match must not reach behind n_bytes): spl_split_device
    against spl_split_host on the n_bytes bytes alone, and spl_encode_batch_device against the Python oracle."""
    import torch
    t, _ = _custom()
    L = _lib()
    wants = {}

    def run(ending, flags, r, c):
        what = f"custom pattern, ending {ending!r}, n_bytes % 16 = {r}"
        if (ending, r) not in wants:
            wants[(ending, r)] = (_custom_want(coracle, c), _host_bits(t, c.blob, c.off))
        want, (st, gp) = wants[(ending, r)]
        words = len(st)
        d_st, d_gp, d_status = Guarded(words, torch.int32), Guarded(words, torch.int32), Guarded(1, torch.int32)
        d_status.view.zero_()
        assert L.spl_split_device(t.handle, c.text.data_ptr(), c.n_bytes, c.d_off.data_ptr(), c.n_docs, d_st.ptr(), d_gp.ptr(), d_status.ptr(), _stream()) == 0
        torch.cuda.synchronize()
        assert d_status.host().tolist() == [0], what
        assert np.array_equal(d_st.host().view(np.uint32), st) and np.array_equal(d_gp.host().view(np.uint32), gp), what
        before = L.spl_device_split_fallbacks(t.handle)
        got = _call(t, c, c.n_bytes, want, what, flags=flags)
        assert L.spl_device_split_fallbacks(t.handle) == before, what
        return got
    _sweep_tails(run)
