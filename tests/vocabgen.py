"""Seeded VOCABULARY families (pure Python, no GPU import): where fuzzgen / stressgen vary the text, these vary the vocabulary, so that the
table builder (splintr_amd/csrc/spl_tables.cpp) produces what the five shipped vocabularies never make it produce, and the probes
(spl_lookup.h) and merge loops read it.  family(name) -> (encoder: dict[bytes, int], texts: list[str]), deterministic; tiktoken(encoder)
serialises an encoder to the reference's on-disk text (`base64 rank` lines, src/core/vocab.rs:57-89).

  prefix_300 / _3000 / _30000   the first k ranks of cl100k_base: closed under their merges -- the control
  permuted_300 / _3000 / _30000 the same keys, their ids shuffled: merge order follows neither length nor training order
  subset_bytes                  the first 30 000 ranks, each multi-byte key kept with p = 0.5: tokens whose 2-splits are no tokens
  subset_nobytes                ... and each single byte dropped with p = 0.6: pseudo ids (max id + 1 + k) in a large vocabulary
  crowd_short                   256 bytes + 3 000 keys of 9..12 bytes under ONE two-byte prefix: a short-table group that finds no salt,
                                full buckets marked SPL_OVF_BIT, probe_short12's walk to the next bucket
  crowd_t8                      3 000 keys of 5..8 bytes under ONE four-byte prefix: one displacement group, the t8 table has to grow
  crowd_long                    3 000 keys of 13..40 bytes that share their first 8 bytes: the long table's linear probing, one p8 entry
  lengths                       two keys at each length of LENGTHS (up to 300 bytes: p8's length byte clamps at 255), sparse ids, the
                                largest id the builder accepts (2^21 - 2) on a key that long runs merge into
"""
import base64
import random

TOP_ID = 2 ** 21 - 2                     # the largest id spl_create accepts (2^21 - 1 would read as an empty pair-table slot)
LENGTHS = (2, 3, 4, 5, 8, 9, 12, 13, 16, 17, 32, 33, 64, 65, 127, 128, 129, 200, 254, 255, 256, 300)
RUN, CUT = "z", "qxj"                    # lengths(): one key of each length is a run of RUN, the other a cut of CUT repeated
_LOWER = "abcdefghijklmnopqrstuvwxyz"


def tiktoken(enc):
    return b"".join(base64.b64encode(k) + b" " + str(v).encode() + b"\n" for k, v in sorted(enc.items(), key=lambda kv: kv[1]))


def holes(enc, limit=200):
    """ids below the largest one that name no key (a sparse family's; a dense one has none)"""
    have = set(enc.values())
    top = max(have)
    if top + 1 == len(have):
        return []
    rng = random.Random(top)
    out = set()
    for _ in range(limit * 50):
        if len(out) >= limit:
            break
        i = rng.randrange(top)
        if i not in have:
            out.add(i)
    return sorted(out)


_cl100k = None


def _cl100k_ranks(k):
    """the first k ranks of cl100k_base, as (key, id) in id order"""
    global _cl100k
    if _cl100k is None:
        from oracle.pyoracle import Oracle
        enc = Oracle.from_pretrained("cl100k_base", engine="regex").encoder
        _cl100k = sorted(enc.items(), key=lambda kv: kv[1])
    assert _cl100k[k - 1][1] == k - 1
    return _cl100k[:k]


def _text_of(b):
    try:
        return b.decode("utf-8")
    except UnicodeDecodeError:
        return None


def _band(rng, frags, lo, hi):
    """a run of letters of lo..hi bytes made of key fragments (so that it merges) and stray letters"""
    n = rng.randrange(lo, hi + 1)
    s = ""
    while len(s) < n:
        s += rng.choice(frags) if rng.random() < 0.8 else rng.choice(_LOWER)
    return s[:n]


def _texts(rng, keys, near, frags, n_mix=160):
    """What every family's texts hold: chunks that are exactly a key, a key plus / minus a byte, near misses, letter chunks of 1..16,
    17..64 and 65..260 bytes, and space-separated mixes of all of them.  keys / near: str; frags: letter-only pieces."""
    keys = list(keys)
    exact = [rng.choice(keys) for _ in range(60)]
    edge = []
    for k in exact[:40]:
        edge += [k[:-1], k + rng.choice(_LOWER), k[1:]] if len(k) > 1 else [k + rng.choice(_LOWER)]
    chunks = ([_band(rng, frags, 1, 16) for _ in range(40)] + [_band(rng, frags, 17, 64) for _ in range(40)]
              + [_band(rng, frags, 65, 260) for _ in range(24)])
    atoms = exact + edge + list(near) + chunks[:80]
    docs = exact[:20] + edge[:10] + list(near)[:10] + exact[20:] + edge[10:] + list(near)[10:] + chunks
    for _ in range(n_mix):
        parts = [rng.choice(atoms) for _ in range(rng.randrange(2, 12))]
        doc = " ".join(parts)
        while len(doc) > 380 and len(parts) > 1:
            parts.pop()
            doc = " ".join(parts)
        docs.append(doc)
    docs += ["", " ", "Hello, world! 123 it's\n\nok", "x  y\t\nz   "]
    return [d for d in docs if d is not None]


# ------------------------------------------------------------------------------------------------
# families made from cl100k_base
# ------------------------------------------------------------------------------------------------
def _cl_texts(rng, enc, universe):
    """Texts for a vocabulary cut from cl100k_base.  `universe`: the keys it was cut FROM -- the dropped ones are the near misses."""
    ks = [t for t in (_text_of(k) for k in enc if len(k) >= 2) if t is not None and "\r" not in t]
    ks.sort()
    sample = rng.sample(ks, min(len(ks), 400))
    dropped = sorted(t for t in (_text_of(k) for k in universe if k not in enc and len(k) >= 2) if t is not None)
    near = rng.sample(dropped, min(len(dropped), 40))
    for k in sample[:40]:                                        # a key with its last character changed
        c = k[:-1] + rng.choice(_LOWER)
        if c.encode("utf-8") not in enc:
            near.append(c)
    frags = sorted({k.strip() for k in ks if k.strip().isascii() and k.strip().isalpha()})
    frags = rng.sample(frags, min(len(frags), 300)) or list(_LOWER)
    return _texts(rng, sample, near, frags)


def prefix(k, seed=1):
    enc = dict(_cl100k_ranks(k))
    return enc, _cl_texts(random.Random(seed * 1000 + k), enc, enc)


def permuted(k, seed=2):
    items = _cl100k_ranks(k)
    rng = random.Random(seed * 1000 + k)
    ids = [v for _, v in items]
    rng.shuffle(ids)
    enc = {key: i for (key, _), i in zip(items, ids)}
    return enc, _cl_texts(rng, enc, enc)


def subset(p=0.5, keep_bytes=True, seed=3):
    items = _cl100k_ranks(30000)
    rng = random.Random(seed * 1000 + (1 if keep_bytes else 0))
    enc = {}
    for key, v in items:
        if len(key) == 1:
            if keep_bytes or rng.random() >= 0.6:
                enc[key] = v
        elif rng.random() < p:
            enc[key] = v
    return enc, _cl_texts(rng, enc, dict(items))


# ------------------------------------------------------------------------------------------------
# crowded tables
# ------------------------------------------------------------------------------------------------
def _crowd(rng, head, lo, hi, n):
    """256 bytes, n keys of lo..hi bytes that begin with `head`, and -- for a hundred of them -- every prefix of two bytes and more, so that
    merges lead up to a crowded key as well as the whole-chunk probe."""
    enc = {bytes([b]): b for b in range(256)}
    keys = set()
    while len(keys) < n:
        keys.add(head + "".join(rng.choice(_LOWER) for _ in range(rng.randrange(lo, hi + 1) - len(head))))
    keys = sorted(keys)
    steps = set()
    for k in rng.sample(keys, 100):
        steps.update(k[:m] for m in range(2, len(k)))
    steps -= set(keys)
    for k in sorted(steps, key=lambda s: (len(s), s)) + keys:
        enc[k.encode()] = len(enc)
    near = []
    while len(near) < 60:
        k = rng.choice(keys)
        c = rng.choice((k[:-1] + rng.choice(_LOWER), k + rng.choice(_LOWER), k[:-1], head + _band(rng, list(_LOWER), 1, hi - len(head))))
        if c.encode() not in enc:
            near.append(c)
    sample = rng.sample(keys, 400)
    return enc, _texts(rng, sample, near, sample[:200] + sorted(steps)[:100])


def crowd_short(n=3000, seed=4):
    return _crowd(random.Random(seed), "qz", 9, 12, n)


def crowd_t8(n=3000, seed=5):
    return _crowd(random.Random(seed), "qzvk", 5, 8, n)


def crowd_long(n=3000, seed=6):
    return _crowd(random.Random(seed), "qzvkwxyj", 13, 40, n)


# ------------------------------------------------------------------------------------------------
# key lengths and the id limit
# ------------------------------------------------------------------------------------------------
def lengths(seed=7):
    """Runs of RUN rank by length (so a long run merges 2 -> 4 -> 8 ... -> 256 bytes, through spans whose p8 bound is the clamped 255), the
    256-byte run holds TOP_ID; the cuts of CUT and the single bytes draw their ids at random from the same sparse pool."""
    rng = random.Random(seed)
    n_run = sum(1 for n in LENGTHS if n <= 256)
    pool = rng.sample(range(TOP_ID), 256 + 2 * len(LENGTHS) - 1)
    run_ids = sorted(rng.sample(pool, n_run - 1)) + [TOP_ID]
    rest = [i for i in pool if i not in set(run_ids)]
    rng.shuffle(rest)
    enc = {}
    for n, i in zip([n for n in LENGTHS if n <= 256], run_ids):
        enc[(RUN * n).encode()] = i
    enc[(RUN * 300).encode()] = rest.pop()
    for n in LENGTHS:
        enc[(CUT * 100)[:n].encode()] = rest.pop()
    for b in range(256):
        enc[bytes([b])] = rest.pop()
    assert not rest and len(enc) == 256 + 2 * len(LENGTHS) and max(enc.values()) == TOP_ID
    keys = [k.decode() for k in enc if len(k) >= 2]
    near = [k[:-1] + "y" for k in keys] + [(CUT * 100)[1:n + 1] for n in LENGTHS]
    docs = _texts(rng, keys, near, [RUN * 2, RUN * 3, RUN * 8, CUT, CUT * 2, CUT[:2], RUN], n_mix=60)
    for n in range(1, 321):
        docs += [c * n for c in RUN + CUT] + [(CUT * 107)[:n]]
    # chunks beyond a wavefront's 512 nodes and at the workgroup loop's 2 048: TOP_ID is the last merge's rank, far to the right
    docs += [RUN * 513, RUN * 700, RUN * 2047, RUN * 2048, "q" * 1792 + RUN * 256, "q" * 250 + RUN * 256 + "q" * 6, RUN * 2100]
    return enc, docs


FAMILIES = {
    "prefix_300": lambda: prefix(300), "prefix_3000": lambda: prefix(3000), "prefix_30000": lambda: prefix(30000),
    "permuted_300": lambda: permuted(300), "permuted_3000": lambda: permuted(3000), "permuted_30000": lambda: permuted(30000),
    "subset_bytes": lambda: subset(0.5, True), "subset_nobytes": lambda: subset(0.5, False),
    "crowd_short": crowd_short, "crowd_t8": crowd_t8, "crowd_long": crowd_long, "lengths": lengths,
}
_made = {}


def family(name):
    """(encoder, texts) of a family, made once per process"""
    if name not in _made:
        _made[name] = FAMILIES[name]()
    return _made[name]
