"""The regex guide, the DEFINITION (include/splintr_hip.h, spl_dfa_index_device / spl_dfa_step_device): a walk byte by byte and a brute
force over every id -- nothing tabulated, nothing incremental.  `toks` is the list of the ORDINARY tokens as tests/heal_ref.py has it; a
table is (trans, accept): trans an integer array [S, 256] whose values >= S are DEAD, accept [S]; a state is (q, constrained, broken,
done)."""
import numpy as np

import heal_ref

DEAD = 0xFFFF
MAX_STATES = 4096
STATE_WORDS = 1
MAX_END = 8
KEEP_FREE, I64 = 2, 4
CON, BRK, DONE = 1 << 16, 1 << 17, 1 << 18
FREE = (0, False, False, False)
BROKEN = (0, False, True, False)

ordinary = heal_ref.ordinary


def table_bytes(trans, accept):
    """uint8 [S * 512 + S]: the table as it lies in memory"""
    return np.concatenate([np.ascontiguousarray(trans, dtype="<u2").view(np.uint8).reshape(-1), np.ascontiguousarray(accept, dtype=np.uint8)])


def n_states(tab):
    return len(tab[1])


def walk(tab, q, data):
    """The state behind the bytes from state q (< S), DEAD as soon as a step is: a value that is no state is DEAD."""
    trans, S = tab[0], n_states(tab)
    for x in data:
        q = int(trans[q][x])
        if q >= S:
            return DEAD
    return q


def begin(start):
    return (int(start), True, False, False)


def load(tab, state):
    """The state as a call reads it: broken wins over done, done over constrained; a constrained q that is no state is broken."""
    q, con, broken, done = state
    if broken:
        return BROKEN
    if done:
        return (q, False, False, True)
    if con:
        return (q, True, False, False) if q < n_states(tab) else BROKEN
    return FREE


def allowed(toks, tab, state, end_ids=()):
    """The ids a constrained state may draw (before the rule "never all zero"): by brute force over every ordinary id."""
    q = state[0]
    ok = {i for i, b in toks if walk(tab, q, b) != DEAD}
    if tab[1][q]:
        ok |= set(end_ids)
    return ok


def settle(toks, tab, state, end_ids=()):
    """The state a call leaves behind a state it arrived at: a constrained state with no id to draw is broken."""
    if state[1] and not allowed(toks, tab, state, end_ids):
        return BROKEN
    return state


def mask(toks, tab, state, n_words, end_ids=()):
    """One mask row of a loaded state: uint32 [n_words]; free, done, broken -- and constrained with nothing to draw -- all ones."""
    ok = allowed(toks, tab, state, end_ids) if state[1] else set()
    if not ok:
        return np.full(n_words, 0xFFFFFFFF, dtype=np.uint32)
    row = np.zeros(n_words, dtype=np.uint32)
    for i in ok:
        row[i >> 5] |= np.uint32(1 << (i & 31))
    return row


def step(toks, tab, state, ids, end_ids=()):
    """The loaded state after the ids, each recomputed from the rule (not settled)."""
    q, con, broken, done = state
    for t in ids:
        if not con:
            break
        b = heal_ref._bytes_of(toks, t)
        q1 = walk(tab, q, b) if b is not None else DEAD
        if q1 != DEAD:
            q = q1
            continue
        con = False
        if t in end_ids and tab[1][q]:
            done = True
        else:
            q, broken = 0, True
    return (q, con, broken, done)


def call(toks, tab, state, ids, n_words, end_ids=()):
    """What one call does to a state word as it lies in memory -> (state written back, mask row)."""
    s = settle(toks, tab, step(toks, tab, load(tab, state), ids, end_ids), end_ids)
    return s, mask(toks, tab, s, n_words, end_ids)


def state_row(state):
    """The canonical word of a state."""
    q, con, broken, done = state
    if broken:
        return BRK
    if done:
        return q | DONE
    return (q | CON) if con else 0


def raw_row(q=0, con=False, broken=False, done=False, extra=0):
    """A word as a caller may write it, canonical or not."""
    return (q & 0xFFFF) | (CON if con else 0) | (BRK if broken else 0) | (DONE if done else 0) | extra


def row_state(word):
    word = int(word)
    return (word & 0xFFFF, bool(word & CON), bool(word & BRK), bool(word & DONE))


def stride(n_words):
    return (n_words + 3) // 4 * 4


def index(toks, tab, n_words):
    """(rows uint32 [S, stride], some uint8 [S]): bit t of row q iff t is ordinary and walk(q, b(t)) is not DEAD; zeros elsewhere."""
    S = n_states(tab)
    rows = np.zeros((S, stride(n_words)), dtype=np.uint32)
    for q in range(S):
        for i, b in toks:
            if walk(tab, q, b) != DEAD:
                rows[q, i >> 5] |= np.uint32(1 << (i & 31))
    return rows, (rows != 0).any(axis=1).astype(np.uint8)
