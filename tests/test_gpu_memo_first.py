"""GPU tests (-m gpu) of the vocabulary-seeded chunk memo and the memo-first probe (csrc/spl_k_memo.h k_memo_seed, csrc/spl_k_pretok.h probe
phase, option "memo_first"): a new memo holds the vocabulary's keys of 2..64 bytes, and the tile kernel asks it before the vocabulary's
tables.  Result-transparent: every pass of every case equals the oracle bit for bit -- seed only, while learned chunks go in (and evict
seeds), warm, with tables too small for the seed, with the options toggled on one handle, through every kind of launch."""
import ctypes
import os

import numpy as np
import pytest

from conftest import VOCABS

pytestmark = pytest.mark.gpu


def _csr(orc, docs, special=False):
    """docs: bytes"""
    off = np.zeros(len(docs) + 1, dtype=np.uint64)
    if docs:
        np.cumsum([len(b) for b in docs], out=off[1:])
    return orc.encode_packed(np.frombuffer(b"".join(docs), dtype=np.uint8), off, special, threads=os.cpu_count() or 8)


def _L():
    from splintr_amd import _ffi
    L = _ffi.lib()
    L.spl_memo_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
    L.spl_memo_seed_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
    return L


def _stats(t):
    o = (ctypes.c_uint64 * 4)()
    assert _L().spl_memo_stats(t.handle, o) == 0
    return list(o)


def _seed(t):
    from splintr_amd import _ffi
    o = (ctypes.c_uint64 * 2)()
    assert _L().spl_memo_seed_stats(t.handle, o) == 0, _ffi.last_error()
    return list(o)


def _opt(t, k, v):
    from splintr_amd import _ffi
    assert _ffi.lib().spl_set_option(t.handle, k.encode(), int(v)) == 0, _ffi.last_error()


def _passes(t, want, texts, n, special=False, what=""):
    for k in range(n):
        ids, off = t.encode_batch_csr(texts, with_special=special)
        assert np.array_equal(off, want[1]) and np.array_equal(ids, want[0]), f"{what} pass {k}"


_keys = {}


def _vocab_keys(name):
    """{id: bytes} in the key space the kernels see"""
    from memo_seed_sim import MemoSeedSim
    if name not in _keys:
        _keys[name] = MemoSeedSim(name).tokens()
    return _keys[name]


@pytest.mark.parametrize("name", VOCABS)
def test_fresh_handle_seed_only_filling_warm(coracle, name):
    from splintr_amd import Tokenizer, corpus
    t = Tokenizer.from_pretrained(name)
    placed, left = _seed(t)
    n_keys = sum(1 for b in _vocab_keys(name).values() if 2 <= len(b) <= 64)
    assert placed > 0 and placed + left == n_keys and left < n_keys // 20, (placed, left, n_keys)
    st = _stats(t)
    assert st[1] == 0 and st[2] == 0 and t.cache_len == 0, st          # seeds are no learned chunks
    texts = corpus.c2_wide(100, seed=177) + corpus.c3(20, seed=178) + corpus.c4(100, seed=179)
    _passes(t, _csr(coracle(name), [x.encode() for x in texts]), texts, 4, what=name)
    assert _seed(t) == [placed, left]


def _entry(t, lng, slot):
    from splintr_amd import _ffi
    L = _L()
    L.spl_debug_memo_entry.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
    o = (ctypes.c_uint32 * 24)()
    assert L.spl_debug_memo_entry(t.handle, lng, slot, o) == 0, _ffi.last_error()
    return list(o)


@pytest.mark.parametrize("name", ["cl100k_base", "deepseek_v3"])
def test_the_seed_lies_in_the_device_s_table_where_the_probe_looks(name):
    """Results stay exact if the seed is useless (every lane falls back to the vocabulary's tables), so this reads the table back: the
    records of the host's plan -- whose slots tests/test_memo_seed_cpu.py checks against the probe's order -- lie in HBM, key zero padded,
    one token, marked as seeds; and a slot the plan leaves empty is empty."""
    from memo_seed_sim import MemoSeedSim
    from splintr_amd import Tokenizer
    t = Tokenizer.from_pretrained(name)
    placed, left = _seed(t)                                             # (a query: no memo yet)
    assert _stats(t)[3] == 0
    assert t.encode("a") != []                                          # one launch: the memo is built and seeded
    assert _stats(t)[3] == (1 << 20) + (1 << 16) and _seed(t) == [placed, left]
    (p2, l2), tabs = MemoSeedSim(name).plan(20, 16)
    assert (p2, l2) == (placed, left)
    rng = np.random.default_rng(5)
    for lng, tab in enumerate(tabs):
        n_rec = len(tab["slot"])
        assert n_rec > 0
        pick = set(rng.choice(n_rec, size=min(n_rec, 150), replace=False).tolist()) | {0, n_rec - 1}
        pick |= set(np.nonzero(tab["slot"] != tab["first"])[0][:50].tolist())                     # keys in their SECOND slot
        for i in sorted(pick):
            e = _entry(t, lng, int(tab["slot"][i]))
            n, key = int(tab["n"][i]), tab["key"][i].tolist()
            assert e[:8] == key[:8] and (not lng or e[16:24] == key[8:16]), (lng, i)
            assert e[8] == (0x80000000 | 0x40000000 | (1 << 8) | (n - 32 if lng else n)) and e[9] == 0 and e[10] == int(tab["id"][i]), (lng, i, hex(e[8]))
        used = set(tab["slot"].tolist())
        free = next(s for s in range(tab["mask"] + 1) if s not in used)
        assert _entry(t, lng, free)[8] == 0


@pytest.mark.parametrize("name", VOCABS)
def test_the_vocabulary_s_own_keys_one_document_each(coracle, name):
    """Keys of 1, 2, 3..32, 33..64 and more than 64 bytes, in first and in second slots.  The oracle is the judge: a key that is one chunk of
    text comes back as its single id; the split pattern cuts a few keys (control tokens such as "[INST]"), those come back as the oracle says."""
    from splintr_amd import Tokenizer
    ids_, docs = [], []
    for tid, b in sorted(_vocab_keys(name).items()):
        try:
            b.decode("utf-8")
        except UnicodeDecodeError:
            continue
        ids_.append(tid)
        docs.append(b)
    lens = {min(len(b), 65) for b in docs}
    assert {1, 2, 3, 32, 33, 64, 65}.issubset(lens) and len(docs) > 30000, sorted(lens)          # (65: more than 64 bytes)
    want = _csr(coracle(name), docs)
    cnt = np.diff(want[1].astype(np.int64))
    single = cnt == 1
    assert single.sum() > len(docs) * 9 // 10
    assert np.array_equal(want[0][want[1][:-1].astype(np.int64)[single]], np.asarray(ids_, dtype=want[0].dtype)[single])
    t = Tokenizer.from_pretrained(name)
    texts = [b.decode("utf-8") for b in docs]
    _passes(t, want, texts, 2, what=name)


def test_window_and_tile_edges(coracle):
    """k filler bytes, then a vocabulary token of 20..64 bytes -- a run of spaces, a run of '=' --, k = 700..1100: the chunk starts at, ends
    at and straddles every position around the 800-byte tile and the 1024-byte window.  Every document alone (its chunk AT k) and all in one batch."""
    from splintr_amd import Tokenizer
    keys = _vocab_keys("cl100k_base")
    runs = {}
    for ch in (b" ", b"="):
        have = sorted(len(b) for b in keys.values() if 20 <= len(b) <= 64 and b == ch * len(b))
        assert have, ch
        runs[ch] = sorted({have[0], have[-1], max([n for n in have if n <= 32], default=have[0]), min([n for n in have if n > 32], default=have[-1])})
    assert any(n > 32 for n in runs[b" "] + runs[b"="]) and any(n <= 32 for n in runs[b" "] + runs[b"="]), runs
    docs = []
    for k in range(700, 1101):
        filler = (b"lorem ipsum dolor sit amet " * 45)[: k - 1] + b"x"
        for ch, ns in runs.items():
            for n in ns:
                docs.append(filler + ch * n)
    orc = coracle("cl100k_base")
    want = _csr(orc, docs)
    texts = [d.decode() for d in docs]
    t = Tokenizer.from_pretrained("cl100k_base")
    assert _seed(t)[0] > 0
    _passes(t, want, texts, 2, what="one batch")
    ids, off = want[0], want[1].astype(np.int64)
    for i, x in enumerate(texts):
        assert t.encode(x) == ids[off[i]:off[i + 1]].tolist(), (i, len(x))


@pytest.mark.parametrize("bits,long_bits", [(4, 4), (8, None)])
def test_tiny_tables_learned_chunks_evict_seeds_and_seeds_never_fit(coracle, bits, long_bits):
    from splintr_amd import Tokenizer, corpus
    t = Tokenizer.from_pretrained("cl100k_base")
    _opt(t, "memo_bits", bits)
    if long_bits is not None:
        _opt(t, "memo_long_bits", long_bits)
    _opt(t, "memo_log_cap", 8)
    placed, left = _seed(t)
    assert 0 < placed <= (1 << bits) + (1 << (long_bits or 16)) and left > 0
    texts = corpus.c2_wide(200, seed=211)
    _passes(t, _csr(coracle("cl100k_base"), [x.encode() for x in texts]), texts, 6, what=f"memo_bits {bits}")
    assert _stats(t)[0] >= 1


def test_toggles_on_one_handle_and_clear_cache(coracle):
    from splintr_amd import Tokenizer, corpus
    t = Tokenizer.from_pretrained("o200k_base")
    texts = corpus.c3(30, seed=231) + corpus.c2_wide(150, seed=232)
    want = _csr(coracle("o200k_base"), [x.encode() for x in texts])
    seed0 = _seed(t)
    for memo_first, memo in ((1, 1), (0, 1), (0, 1), (1, 1), (1, 0), (1, 1), (1, 1), (0, 0), (0, 1), (1, 1), (1, 1)):
        _opt(t, "memo_first", memo_first)
        _opt(t, "memo", memo)
        _passes(t, want, texts, 1, what=f"memo_first {memo_first} memo {memo}")
    _passes(t, want, texts, 3)
    assert t.cache_len > 0
    t.clear_cache()
    assert t.cache_len == 0 and _stats(t)[1] == 0
    assert _seed(t) == seed0 and seed0[0] > 0
    assert t.cache_len == 0
    _passes(t, want, texts, 3, what="behind clear_cache")
    _opt(t, "memo_first", 0)
    assert _seed(t) == [0, 0]                                          # an unseeded memo
    _passes(t, want, texts, 2, what="memo_first 0")


def test_special_tokens_through_the_seeded_memo(coracle):
    from splintr_amd import Tokenizer, corpus
    t = Tokenizer.from_pretrained("cl100k_base")
    base = corpus.c2_wide(120, seed=241)
    texts = [x[: len(x) // 2] + "<|endoftext|>" + x[len(x) // 2:] for x in base]
    orc = coracle("cl100k_base")
    for sp in (True, False, True, True):
        _passes(t, _csr(orc, [x.encode() for x in texts], sp), texts, 1, special=sp, what=f"special {sp}")


def test_a_gpt2_pattern_handle_with_external_boundaries():
    from splintr_amd import corpus
    from test_gpu_custom_pattern import _check, _pair
    from test_host_regex import GPT2_PATTERN
    t, orc = _pair("cl100k_base", GPT2_PATTERN)
    assert t.has_custom_pattern and _seed(t)[0] > 0
    texts = corpus.c2_wide(60, seed=251) + corpus.c2(40, seed=252) + ["", "a", " ", "it's 1234567 x" * 9]
    for _ in range(3):
        _check(t, orc, texts)


def test_single_texts_through_a_seeded_memo(coracle):
    from splintr_amd import Tokenizer, corpus
    t = Tokenizer.from_pretrained("llama3")
    orc = coracle("llama3")
    texts = corpus.c2_wide(120, seed=261) + ["", "a", "\n", "é", "Hello, world!", "x" * 70, " " * 300]
    want = orc.encode_batch(texts)
    for rnd in range(2):
        for x, w in zip(texts, want):
            assert t.encode(x) == w, (rnd, x[:60])


def test_a_vocabulary_that_lacks_single_bytes():
    """tests/vocabgen.py subset_nobytes: a one-byte chunk whose byte is no token has a pseudo id and yields no token -- by byte_id directly
    with the memo first."""
    import vocabgen
    from splintr_amd import CL100K_BASE_PATTERN, Tokenizer
    from oracle.pyoracle import Oracle
    enc, texts = vocabgen.family("subset_nobytes")
    missing = [b for b in range(0x21, 0x7F) if bytes([b]) not in enc]
    assert missing
    texts = list(texts) + [chr(b) for b in missing] + [" ".join(chr(b) for b in missing), "\n".join(chr(b) + "!" for b in missing)]
    orc = Oracle(enc, CL100K_BASE_PATTERN, False)
    want = [orc.encode(x) for x in texts]
    assert any(w == [] for w in want[-len(missing) - 2:-2])
    t = Tokenizer.from_bytes(vocabgen.tiktoken(enc), CL100K_BASE_PATTERN)
    assert _seed(t)[0] > 0
    for phase in ("seed only", "filling", "warm"):
        got = t.encode_batch(texts)
        bad = [i for i in range(len(texts)) if got[i] != want[i]]
        assert not bad, (phase, len(bad), texts[bad[0]][:60], got[bad[0]][:12], want[bad[0]][:12])
    _opt(t, "memo_first", 0)
    assert t.encode_batch(texts) == want
