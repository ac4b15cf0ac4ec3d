"""GPU tests (-m gpu): the generated vocabulary families of tests/vocabgen.py through the kernels, against oracle/pyoracle.py.
Every family twice -- with the cl100k_base pattern (the SCANNER path of k_pretok, which only the five shipped vocabularies had taken) and
with the custom pattern of test_gpu_vocab_shapes.py (the device splitter) --: three batch passes (chunk memo cold, filling, warm), the
latency path, the forced tile geometry B; and decode, whose table is built from the same vocabulary.  What each family makes the table
builder produce is asserted on the CPU (tests/test_vocab_generated_cpu.py)."""
import ctypes
import random

import pytest

import vocabgen

pytestmark = pytest.mark.gpu

CUSTOM = r"[a-z]+|\s+|[^a-z\s]+"
WHICH = ("scanner", "custom")
GEOM_FAMILIES = ("subset_bytes", "subset_nobytes", "crowd_short", "crowd_t8", "crowd_long", "lengths")

_oracles, _toks = {}, {}


def _pattern(which):
    from splintr_amd import CL100K_BASE_PATTERN
    return CL100K_BASE_PATTERN if which == "scanner" else CUSTOM


def _oracle(name, which):
    """(oracle, ids of the family's texts), made once; the two patterns of a family share the oracle's memo of merged chunks"""
    if (name, which) not in _oracles:
        from oracle.pyoracle import Oracle
        enc, texts = vocabgen.family(name)
        orc = Oracle(enc, _pattern(which), False)
        for w in WHICH:
            if (name, w) in _oracles:
                orc._chunk_memo = _oracles[(name, w)][0]._chunk_memo
        _oracles[(name, which)] = (orc, [orc.encode(x) for x in texts])
    return _oracles[(name, which)]


def _tok(name, which):
    if (name, which) not in _toks:
        from splintr_amd import Tokenizer
        _toks[(name, which)] = Tokenizer.from_bytes(vocabgen.tiktoken(vocabgen.family(name)[0]), _pattern(which))
    return _toks[(name, which)]


def _force_tiles(t, mode):
    """test_gpu_parity._force_tiles on a handle of our own: 0 the size decides, 5 tile-owned geometry B (864 + 128) at any size"""
    from splintr_amd import _ffi
    st = (ctypes.c_uint64 * 16)()
    assert _ffi.lib().spl_debug_phases(t.handle, mode << 1, st) == 0


def _same(got, want, texts, what):
    if got != want:
        bad = [i for i in range(len(texts)) if got[i] != want[i]]
        i = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(texts)} documents differ; first #{i} {texts[i][:100]!r} ({len(texts[i])} chars): "
                             f"{got[i][:16]} vs {want[i][:16]}")


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("name", list(vocabgen.FAMILIES))
def test_family_encodes_as_the_oracle(name, which):
    enc, texts = vocabgen.family(name)
    _, want = _oracle(name, which)
    t = _tok(name, which)
    assert t.has_custom_pattern == (which == "custom") and t.vocab_size == max(enc.values()) + 1
    for phase in ("memo cold", "memo filling", "memo warm"):
        _same(t.encode_batch(texts), want, texts, f"{name}, {which}, {phase}")
    for x, w in list(zip(texts, want))[:40]:
        assert t.encode(x) == w, (name, which, x)
    if name in GEOM_FAMILIES:
        try:
            for geom in (5, 0):
                _force_tiles(t, geom)
                t.clear_cache()
                for phase in ("memo cold", "memo filling"):
                    _same(t.encode_batch(texts), want, texts, f"{name}, {which}, geometry {geom}, {phase}")
        finally:
            _force_tiles(t, 0)


@pytest.mark.parametrize("name", list(vocabgen.FAMILIES))
def test_family_decodes_as_the_oracle(name):
    enc, texts = vocabgen.family(name)
    orc, want = _oracle(name, "scanner")
    t = _tok(name, "scanner")
    top = max(enc.values())
    rng = random.Random(top)
    streams = list(want)
    streams += [[rng.randrange(top + 2) for _ in range(rng.randrange(1, 400))] for _ in range(50)]     # (top + 1: beyond the table)
    known = sorted(enc.values())
    streams += [[rng.choice(known) for _ in range(rng.randrange(1, 200))] for _ in range(50)]
    hole = vocabgen.holes(enc)
    if name in ("subset_bytes", "subset_nobytes", "lengths"):
        assert len(hole) == 200
    if hole:
        assert orc.decode_bytes(hole) == b""
        streams += [hole, [top] + hole[:3] + [known[0]] + hole[3:6] + [top + 1, top]]
    got = t._decode_batch_bytes(streams)
    for i, s in enumerate(streams):
        assert got[i] == orc.decode_bytes(s), (name, i, s[:16])
    for x, w, g in zip(texts, want, got):
        if len({bytes([b]) for b in x.encode("utf-8")} - set(enc)) == 0:          # every byte is a token: the text comes back
            assert g == x.encode("utf-8"), (name, x)


RUNS = (2, 3, 4, 8, 9, 16, 17, 32, 33, 64, 65, 128, 160, 700)


def test_the_id_limit_on_the_device():
    """b"zz" -> 2^21 - 1 is refused (its pair with itself reads as an empty pair-table slot: ids 4194303 came out); b"zz" -> 2^21 - 2, the
    largest id, encodes runs of z exactly on the batch path and the latency path."""
    from oracle.pyoracle import Oracle
    from splintr_amd import Tokenizer
    for which in WHICH:
        enc = {bytes([b]): b for b in range(256)}
        enc[b"zz"] = 2 ** 21 - 1
        with pytest.raises(ValueError, match=r"token ids must be < 2\^21 - 1"):
            Tokenizer.from_bytes(vocabgen.tiktoken(enc), _pattern(which))
        enc[b"zz"] = top = 2 ** 21 - 2
        t = Tokenizer.from_bytes(vocabgen.tiktoken(enc), _pattern(which))
        texts = ["z" * n for n in RUNS] + [" ".join("z" * n for n in RUNS)]
        orc = Oracle(enc, _pattern(which), False)
        want = [orc.encode(x) for x in texts]
        assert want[:-1] == [[top] * (n // 2) + [ord("z")] * (n % 2) for n in RUNS]
        assert want[-1] == [x for i, w in enumerate(want[:-1]) for x in ([32] if i else []) + w]    # (a blank merges with nothing)
        for _ in range(3):
            assert t.encode_batch(texts) == want, which
        for x, w in zip(texts, want):
            assert t.encode(x) == w, (which, len(x))
        assert t.vocab_size == top + 1 and t._decode_batch_bytes([want[-1]]) == [texts[-1].encode()]
