"""Guided choice, the DEFINITION (include/splintr_hip.h, spl_choice_step_device): bytes.startswith over lists -- nothing sorted, nothing
incremental.  `toks` is the list of the ORDINARY tokens as tests/heal_ref.py has it; `choices` a list of 64 byte strings or fewer (b"": an
empty slot); a state is (A, k, broken, done, hit) with A a frozenset of slots."""
import numpy as np

import heal_ref

SLOTS = 64
MAX_LEN = 64
STATE_WORDS = 2
MAX_END = 8
TABLE_BYTES = SLOTS * MAX_LEN + SLOTS
THEN_FREE, KEEP_FREE, I64 = 1, 2, 4
FREE = (frozenset(), 0, False, False, 0)
BROKEN = (frozenset(), 0, True, False, 0)

ordinary = heal_ref.ordinary


def table(choices, lens=None):
    """uint8 [4160]: slot s = choices[s]; lens overrides the length bytes (a table no builder makes: lengths above 64)"""
    tab = np.zeros(TABLE_BYTES, dtype=np.uint8)
    for s, c in enumerate(choices):
        assert len(c) <= MAX_LEN
        tab[MAX_LEN * s:MAX_LEN * s + len(c)] = np.frombuffer(bytes(c), dtype=np.uint8)
        tab[SLOTS * MAX_LEN + s] = len(c)
    if lens is not None:
        tab[SLOTS * MAX_LEN:SLOTS * MAX_LEN + len(lens)] = lens
    return tab


def begin(choices, selection=None):
    """The state a caller writes: the selected slots (None: all of them), nothing spelled."""
    return (frozenset(range(len(choices)) if selection is None else selection), 0, False, False, 0)


def load(choices, state):
    """The state as a call reads it: k clamped, done and broken rows without slots, slots that cannot be spelled from k dropped."""
    A, k, broken, done, hit = state
    k = min(k, MAX_LEN)
    if broken:
        return BROKEN
    if done:
        return (frozenset(), k, False, True, hit)
    A = frozenset(s for s in A if s < len(choices) and 1 <= len(choices[s]) <= MAX_LEN and len(choices[s]) >= k)
    return (A, k, False, False, 0) if A else FREE


def rests(choices, state):
    A, k = state[0], state[1]
    return {s: choices[s][k:] for s in A}


def allowed(toks, choices, state, end_ids=(), then_free=False):
    """The ids a constrained state may draw (before the rule "never all zero")."""
    r = rests(choices, state)
    ok = {i for i, b in toks if any(len(b) <= len(x) and x.startswith(b) for x in r.values())}
    if not then_free and any(len(x) == 0 for x in r.values()):
        ok |= set(end_ids)
    return ok


def settle(toks, choices, state, end_ids=(), then_free=False):
    """The state a call leaves behind a state it arrived at: a constrained state with no id to draw is broken."""
    if state[0] and not allowed(toks, choices, state, end_ids, then_free):
        return BROKEN
    return state


def mask(toks, choices, state, n_words, end_ids=(), then_free=False):
    """One mask row of a loaded state: uint32 [n_words]; free, done, broken -- and constrained with nothing to draw -- all ones."""
    ok = allowed(toks, choices, state, end_ids, then_free) if state[0] else set()
    if not ok:
        return np.full(n_words, 0xFFFFFFFF, dtype=np.uint32)
    row = np.zeros(n_words, dtype=np.uint32)
    for i in ok:
        row[i >> 5] |= np.uint32(1 << (i & 31))
    return row


def step(toks, choices, state, ids, end_ids=(), then_free=False):
    """The loaded state after the ids, each recomputed from the rule (not settled)."""
    A, k, broken, done, hit = state
    for t in ids:
        if not A:
            break
        b = heal_ref._bytes_of(toks, t)
        S = frozenset(s for s in A if choices[s][k:].startswith(b)) if b is not None else frozenset()
        if S:
            A, k = S, k + len(b)
            if then_free and any(len(choices[s]) == k for s in A):
                done, hit, A = True, min(s for s in A if len(choices[s]) == k), frozenset()
            continue
        E = [s for s in A if len(choices[s]) == k] if (not then_free and t in end_ids) else []
        if E:
            done, hit, A = True, min(E), frozenset()
        else:
            A, k, broken = frozenset(), 0, True
    return (A, k, broken, done, hit)


def call(toks, choices, state, ids, n_words, end_ids=(), then_free=False):
    """What one call does to a row as it lies in memory -> (state written back, mask row)."""
    s = settle(toks, choices, step(toks, choices, load(choices, state), ids, end_ids, then_free), end_ids, then_free)
    return s, mask(toks, choices, s, n_words, end_ids, then_free)


def state_row(state):
    """The canonical row of a state."""
    A, k, broken, done, hit = state
    row = np.zeros(STATE_WORDS, dtype=np.uint64)
    if broken:
        row[1] = 1 << 8
    elif done:
        row[1] = k | (1 << 9) | (hit << 16)
    elif A:
        row[0] = sum(1 << s for s in A)
        row[1] = k
    return row


def raw_row(A, k=0, broken=False, done=False, hit=0):
    """A row as a caller may write it, canonical or not."""
    return np.array([sum(1 << s for s in A), k | (int(broken) << 8) | (int(done) << 9) | (hit << 16)], dtype=np.uint64)


def row_state(row):
    row = np.asarray(row, dtype=np.uint64)
    w0, w1 = int(row[0]), int(row[1])
    return (frozenset(s for s in range(SLOTS) if (w0 >> s) & 1), w1 & 0x7F, bool((w1 >> 8) & 1), bool((w1 >> 9) & 1), (w1 >> 16) & 63)
