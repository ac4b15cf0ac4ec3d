"""Toy vocabularies and inputs shared by tests/test_heal_cpu.py (the host simulation) and tests/test_gpu_heal.py (the kernels): small enough
for tests/heal_ref.py to enumerate, shaped so that every edge of the search and of the chain is met."""
import itertools
import random

import numpy as np

import heal_ref as ref


def vocab_chain():
    """Every string of up to 3 bytes over {a, b}, plus "a" * k for k = 4 .. 64: a partial chain of depth 63."""
    toks = [bytes(t) for n in (1, 2, 3) for t in itertools.product(b"ab", repeat=n)] + [b"a" * k for k in range(4, 65)]
    return dict(enumerate(toks)), {}


def vocab_gaps():
    """Lacks the single bytes b and c, has id gaps, a special inside the dense range that spells an ordinary token's bytes, and specials
    beyond the range."""
    vocab = {0: b"a", 2: b"ab", 3: b"abc", 5: b"ca", 6: b"cab", 9: b"bb", 10: b"bc", 12: b"aab", 13: b"ba", 17: b"cc", 18: b"ccc",
             19: b"abca", 23: b"bcb", 30: b"aa", 33: b"abcab", 34: b"cabca"}
    specials = {4: b"<s>", 7: b"ab", 20: b"c", 40: b"a", 41: b"<e>"}
    return vocab, specials


def vocab_edges():
    """The smallest and the largest entries are 00 and ff ff: lo = 0, lo = n and prefixes of ff bytes meet the edges of the order."""
    toks = [b"\x00", b"\xff\xff", b"\xff", b"a", b"ab", b"b", b"c\xff", b"cc", b"\x00\x00", b"\xfe", b"abc", b"bca", b"\xff\x00"]
    return dict(enumerate(toks)), {}


def vocab_long():
    """"a" * k for k = 1 .. 65 and 128, and a^63 b: |P| = 63 and 64, 63 partial ids, covering tokens longer than a prefix can be."""
    toks = [b"a" * k for k in range(1, 66)] + [b"a" * 128, b"a" * 63 + b"b", b"b"]
    return dict(enumerate(toks)), {}


TOYS = {"chain": vocab_chain, "gaps": vocab_gaps, "edges": vocab_edges}
EDGE_PREFIXES = [b"\x00", b"\x00\x00", b"\x00\x01", b"\xff", b"\xff\xff", b"\xff\xff\xff", b"\xfe\xff", b"\xff\x00", b"c\xff\xff"]


def prefixes(name):
    ps = [bytes(t) for n in range(1, 6) for t in itertools.product(b"abc", repeat=n)]
    return ps + (EDGE_PREFIXES if name == "edges" else [])


def state_rows(ps):
    """State rows [len(ps), 9] uint64 for fresh sequences with the given pending prefixes (b"": free)."""
    return np.stack([ref.state_row((p, False, False)) for p in ps]) if len(ps) else np.zeros((0, ref.STATE_WORDS), dtype=np.uint64)


def probe_ids(vocab, specials):
    """Every id worth stepping with: the vocabulary, the specials, a gap, the id behind the largest, far beyond, and all-ones."""
    top = max(vocab)
    return sorted(set(vocab) | set(specials) | {top + 1, top + 1000, 0xFFFFFFFF} | {i for i in range(top) if i not in vocab})


def step_cases(name, seed=7, per_prefix=3, length=4):
    """(prefix, ids) pairs: per prefix a few id sequences, half of them spelled along the prefix (so they heal), half random."""
    vocab, specials = TOYS[name]()
    toks = ref.ordinary(vocab)
    rng = random.Random(seed)
    pool = probe_ids(vocab, specials)
    out = []
    for p in prefixes(name):
        for k in range(per_prefix):
            ids, P = [], p
            for _ in range(length):
                ok = sorted(ref.allowed(toks, P)) if P else []
                if ok and (k == 0 or rng.random() < 0.6):
                    t = rng.choice(ok)
                else:
                    t = rng.choice(pool)
                ids.append(t)
                P = ref.step(toks, (P, False, False), [t])[0]
            out.append((p, ids))
    return out


def prompts(name, n=120, seed=11):
    vocab, specials = TOYS[name]()
    rng = random.Random(seed)
    pool = sorted(vocab) * 4 + probe_ids(vocab, specials)
    return [[rng.choice(pool) for _ in range(rng.randrange(0, 8))] for _ in range(n)]


def rows_of(seqs, K, dtype, side="right", pad=0x7FFFFFFF):
    """Sequences as rows [len(seqs), K] of dtype with lengths int32; padding holds an id of no map."""
    a = np.full((len(seqs), K), pad, dtype=np.uint64)
    for i, s in enumerate(seqs):
        if len(s):
            if side == "right":
                a[i, :len(s)] = s
            else:
                a[i, K - len(s):] = s
    a = a.astype(np.uint32).view(np.int32) if dtype == np.int32 else a.astype(np.int64)
    return np.ascontiguousarray(a.reshape(len(seqs), K)), np.array([len(s) for s in seqs], dtype=np.int32)
