"""The chunk memo's seed, without a GPU (csrc/spl_tables.cpp memo_seed_plan through tests/hostsim/memo_seed_sim): where the host puts the
vocabulary's keys of 2..64 bytes in a new memo.  The tile kernel's memo_probe looks at a chunk's first slot and at its second only where
the first holds another chunk, so a placed key must sit exactly there; its id must be what the vocabulary's own tables and the oracle
say; no slot may be written twice; and every key is either placed or counted as left out."""
import numpy as np
import pytest

from conftest import VOCABS

_sims = {}


def _sim(name):
    from memo_seed_sim import MemoSeedSim
    if name not in _sims:
        s = MemoSeedSim(name)
        _sims[name] = (s, s.tokens())
    return _sims[name]


def _key_bytes(rec_words, n):
    return rec_words.astype("<u4").tobytes()[:n]


@pytest.mark.parametrize("bits,long_bits", [(20, 16), (4, 4)])
@pytest.mark.parametrize("name", VOCABS)
def test_placement(coracle, name, bits, long_bits):
    sim, toks = _sim(name)
    (placed, left), tabs = sim.plan(bits, long_bits)
    keys_2_64 = sum(1 for b in toks.values() if 2 <= len(b) <= 64)
    assert placed + left == keys_2_64 and placed > 0
    assert placed == len(tabs[0]["slot"]) + len(tabs[1]["slot"])
    if bits == 4:
        assert placed <= 32                                            # what fits, and no more
    else:
        assert left < keys_2_64 // 20, (placed, left)                  # a table of a million entries holds nearly all of them
    docs, want = [], []
    for lng, t in enumerate(tabs):
        slot, first, second = t["slot"].astype(np.int64), t["first"].astype(np.int64), t["second"].astype(np.int64)
        assert (slot <= t["mask"]).all()
        assert len(np.unique(slot)) == len(slot)                       # no slot written twice
        at_first = slot == first
        # the second slot only where the first holds ANOTHER key (slots are unique: "taken and not mine")
        assert (at_first | ((slot == second) & np.isin(first, slot))).all()
        assert (t["probed"] == t["id"]).all()                          # the whole-chunk tables answer the same id
        assert (np.diff(t["id"].astype(np.int64)) > 0).all()           # ascending ids: the low ids chose first
        lo, hi = (33, 64) if lng else (2, 32)
        assert ((t["n"] >= lo) & (t["n"] <= hi)).all()
        for i in range(len(slot)):
            n, tid = int(t["n"][i]), int(t["id"][i])
            kb = _key_bytes(t["key"][i], n)
            assert kb == toks[tid], tid                                # the key as the probe builds it: the token's bytes ...
            assert not t["key"][i].astype("<u4").tobytes()[n:].strip(b"\0")   # ... zero padded
            docs.append(kb)
            want.append(tid)
    # the oracle: a key that is one chunk of text encodes to its id (a key the split pattern cuts -- few -- is no whole chunk of any text)
    valid = []
    for k, (d, tid) in enumerate(zip(docs, want)):
        try:
            d.decode("utf-8")
            valid.append(k)
        except UnicodeDecodeError:
            pass
    orc = coracle(name)
    off = np.zeros(len(valid) + 1, dtype=np.uint64)
    np.cumsum([len(docs[k]) for k in valid], out=off[1:])
    ids, ooff = orc.encode_packed(np.frombuffer(b"".join(docs[k] for k in valid), dtype=np.uint8), off, False, threads=4)
    cnt = np.diff(ooff.astype(np.int64))
    single = cnt == 1
    got = ids[ooff[:-1].astype(np.int64)[single]]
    assert np.array_equal(got, np.asarray([want[k] for k in valid], dtype=got.dtype)[single])
    cut = [valid[j] for j in np.nonzero(~single)[0]]
    # (a tenth at the most over a whole vocabulary; the sixteen-entry table holds the lowest ids alone, which in mistral_v3 are control
    #  tokens such as "[INST]": keys, but never a chunk)
    assert bits == 4 or len(cut) <= len(valid) // 10, (len(cut), len(valid))
    for k in cut[:2000]:
        assert len(orc.split_bytes(docs[k])) > 1, docs[k]              # (the chunk STARTS: more than one chunk)
