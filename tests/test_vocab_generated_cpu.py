"""Generated vocabularies (tests/vocabgen.py) through the table builder and the shared probe / merge code on the CPU (tests/hostsim)
against the literal restatement of the reference (oracle/pyoracle.py) -- and the id limit: 2^21 - 2 is the largest id a vocabulary may hold,
because the pair (2^21 - 1, 2^21 - 1) has the 42-bit key of an empty pair-table slot.  The GPU side: tests/test_gpu_vocab_generated.py."""
import pytest

import vocabgen
from hostsim import HostSim

_cache = {}


def _sim(name, tmp_path_factory):
    if name not in _cache:
        from oracle.pyoracle import Oracle
        from splintr_amd.tokenizer import CL100K_BASE_PATTERN
        enc, texts = vocabgen.family(name)
        path = tmp_path_factory.mktemp("vocab") / (name + ".tiktoken")
        path.write_bytes(vocabgen.tiktoken(enc))
        _cache[name] = (HostSim.from_file(path, 0), Oracle(enc, CL100K_BASE_PATTERN, False), enc, texts)
    return _cache[name]


def _pow2_at_least(n):
    c = 16
    while c < n:
        c <<= 1
    return c


@pytest.mark.parametrize("name", list(vocabgen.FAMILIES))
def test_family_encodes_as_the_oracle(tmp_path_factory, name):
    h, orc, enc, texts = _sim(name, tmp_path_factory)
    assert h.info()["n_keys"] == len(enc)
    assert h.row_head_check()["violations"] == 0
    assert 100 < len(texts) and max(len(t.encode("utf-8")) for t in texts) <= (2100 if name == "lengths" else 400)
    for text in texts:
        b = text.encode("utf-8")
        assert h.encode(b) == orc.encode_bytes(b), (name, text)


def test_families_reach_the_table_shapes_they_are_for(tmp_path_factory):
    """Conditions on the GENERATOR (a seed that stops meeting one is changed, not the condition)."""
    h = _sim("crowd_short", tmp_path_factory)[0]
    st = h.bucket_stats()
    assert st["unsalted_groups"] >= 1 and st["short"][1] >= 1, st           # a group without a salt, buckets marked overflowed
    h = _sim("crowd_t8", tmp_path_factory)[0]
    slots, keys = h.bucket_stats()["t8"]
    assert keys >= 3000 and slots > _pow2_at_least(max(keys + keys // 4 + 2, 1 << 12)), (slots, keys)   # the table was doubled
    h = _sim("crowd_long", tmp_path_factory)[0]
    assert h.info()["max_key_len"] == 40 and h.info()["long_cap"] >= 2 * 3000
    h, _, enc, _ = _sim("lengths", tmp_path_factory)
    assert h.info()["max_key_len"] == 300 and h.info()["max_id"] == vocabgen.TOP_ID == 2 ** 21 - 2
    assert len(vocabgen.holes(enc)) == 200                                     # sparse
    enc = _sim("subset_nobytes", tmp_path_factory)[2]
    assert 50 < sum(1 for k in enc if len(k) == 1) < 256
    enc = _sim("subset_bytes", tmp_path_factory)[2]
    assert sum(1 for k in enc if len(k) == 1) == 256
    assert any(all(k[:c] not in enc or k[c:] not in enc for c in range(1, len(k))) for k in enc if len(k) > 2)   # not closed under merges
    enc = _sim("permuted_3000", tmp_path_factory)[2]
    assert sorted(enc.values()) == list(range(3000)) and enc != _sim("prefix_3000", tmp_path_factory)[2]


# ------------------------------------------------------------------------------------------------
# the id limit
# ------------------------------------------------------------------------------------------------
RUNS = (2, 3, 4, 8, 9, 16, 17, 32, 33, 64, 65, 128, 700)


def _zz(top, without=()):
    enc = {bytes([b]): b for b in range(256) if b not in without}
    enc[b"zz"] = top
    return enc


def test_id_2_21_minus_1_is_refused_by_the_builder(tmp_path):
    path = tmp_path / "top.tiktoken"
    path.write_bytes(vocabgen.tiktoken(_zz(2 ** 21 - 1)))
    with pytest.raises(ValueError, match=r"token ids must be < 2\^21 - 1"):
        HostSim.from_file(path, 0)
    path.write_bytes(vocabgen.tiktoken(_zz(2 ** 21)))
    with pytest.raises(ValueError, match="21 bits"):
        HostSim.from_file(path, 0)


def test_id_2_21_minus_2_encodes_runs_of_the_pair_exactly(tmp_path):
    from oracle.pyoracle import Oracle
    from splintr_amd.tokenizer import CL100K_BASE_PATTERN
    enc = _zz(2 ** 21 - 2)
    path = tmp_path / "top.tiktoken"
    path.write_bytes(vocabgen.tiktoken(enc))
    h = HostSim.from_file(path, 0)
    assert h.info()["max_id"] == 2 ** 21 - 2
    orc = Oracle(enc, CL100K_BASE_PATTERN, False)
    for n in RUNS:
        b = b"z" * n
        want = orc.encode_bytes(b)
        assert want == [2 ** 21 - 2] * (n // 2) + [ord("z")] * (n % 2)
        assert h.encode(b) == want, n


def test_id_2_21_minus_2_with_a_missing_byte_is_refused(tmp_path):
    """The pseudo id of the missing byte would be 2^21 - 1."""
    path = tmp_path / "top.tiktoken"
    path.write_bytes(vocabgen.tiktoken(_zz(2 ** 21 - 2, without=(7,))))
    with pytest.raises(ValueError, match=r"token ids must be < 2\^21 - 1 \(with the pseudo ids"):
        HostSim.from_file(path, 0)
    path.write_bytes(vocabgen.tiktoken(_zz(2 ** 21 - 3, without=(7,))))         # one lower: the pseudo id is 2^21 - 2
    assert HostSim.from_file(path, 0).encode(b"zzzz\x07z") == [2 ** 21 - 3] * 2 + [ord("z")]


def test_from_bytes_raises_value_error_at_the_id_limit():
    """Tokenizer.from_bytes: the builder runs before anything touches a GPU, so the refusal needs none."""
    from splintr_amd import Tokenizer, CL100K_BASE_PATTERN
    with pytest.raises(ValueError, match=r"token ids must be < 2\^21 - 1"):
        Tokenizer.from_bytes(vocabgen.tiktoken(_zz(2 ** 21 - 1)), CL100K_BASE_PATTERN)
    with pytest.raises(ValueError, match=r"with the pseudo ids"):
        Tokenizer.from_bytes(vocabgen.tiktoken(_zz(2 ** 21 - 2, without=(0, 255))), r"[a-z]+|\s+|[^a-z\s]+")
