"""Token healing, the DEFINITION (include/splintr_hip.h, spl_heal_*_device): bytes.startswith over a list of (id, bytes) -- nothing sorted,
nothing incremental.  `toks` is the list of the ORDINARY tokens: ids of the vocabulary proper with at least one byte (specials, missing ids
and ids above the largest one are simply not in it).  A state is (P, broken, healed)."""
import numpy as np

STATE_WORDS = 9
MAX_PREFIX = 64
FREE = (b"", False, False)


def ordinary(vocab):
    """[(id, bytes)] of a vocabulary proper (a dict or pairs) -> the ordinary tokens."""
    items = vocab.items() if hasattr(vocab, "items") else vocab
    return [(int(i), bytes(b)) for i, b in items if len(b) >= 1]


_by_id = {}


def _bytes_of(toks, t):
    """The bytes of id t if it is in the list (an ordinary token), else None.  The id -> bytes view of one list is kept (a large list is
    asked many times); it holds no order."""
    d = _by_id.get(id(toks))
    if d is None or d[0] is not toks:
        d = _by_id[id(toks)] = (toks, dict(toks))
        assert len(d[1]) == len(toks), "an id twice"
    return d[1].get(t)


def allowed(toks, P):
    """The ids a constrained sequence may draw (P non-empty): covering or partial."""
    assert len(P) >= 1
    return {i for i, b in toks if b.startswith(P) or (P.startswith(b) and len(b) < len(P))}


def mask_words(toks, P, n_words):
    """One mask row: uint32 [n_words], bit t & 31 of word t >> 5; free: all ones."""
    if not P:
        return np.full(n_words, 0xFFFFFFFF, dtype=np.uint32)
    row = np.zeros(n_words, dtype=np.uint32)
    for i in allowed(toks, P):
        row[i >> 5] |= np.uint32(1 << (i & 31))
    return row


def step(toks, state, ids):
    """The state after the ids, each recomputed from the rule."""
    P, broken, healed = state
    for t in ids:
        if not P:
            break                                   # free stays free
        b = _bytes_of(toks, t)
        if b is None:                               # a special, a missing id, an id out of range, -1
            P, broken = b"", True
        elif b.startswith(P):
            P, healed = b"", True
        elif P.startswith(b) and len(b) < len(P):
            P = P[len(b):]
        else:
            P, broken = b"", True
    return (P, broken, healed)


def begin(toks, ids, *, max_back, min_keep=0, auto=False):
    """(n_back, P) for one prompt (its valid ids)."""
    P, j = b"", 1
    while True:
        if j > max_back or len(ids) - j < min_keep:
            break
        b = _bytes_of(toks, ids[len(ids) - j])
        if b is None or len(b) + len(P) > MAX_PREFIX:
            break
        cand = b + P
        if auto and not any(x.startswith(cand) and len(x) > len(cand) for _, x in toks):
            break
        P, j = cand, j + 1
    return j - 1, P


def state_row(state):
    P, broken, healed = state
    assert len(P) <= MAX_PREFIX
    row = np.zeros(STATE_WORDS, dtype=np.uint64)
    row[0] = len(P) | (int(broken) << 8) | (int(healed) << 9)
    row[1:] = np.frombuffer(P + b"\0" * (MAX_PREFIX - len(P)), dtype="<u8")
    return row


def row_state(row):
    row = np.asarray(row, dtype=np.uint64)
    w0 = int(row[0])
    n = w0 & 0x7F
    return (row[1:].astype("<u8").tobytes()[:n], bool((w0 >> 8) & 1), bool((w0 >> 9) & 1))
