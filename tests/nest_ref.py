"""The nest guide, the DEFINITION (include/splintr_hip.h, spl_nest_index_device / spl_nest_step_device): a walk byte by byte over a
configuration (q, stack) and a brute force over every id -- nothing tabulated, nothing incremental -- over the helpers of
tests/dfa_ref.py.  `toks` is the list of the ORDINARY tokens as tests/heal_ref.py has it; a table is (trans [S, 256], ret [n_ret, 16],
op [S, 256], accept [S]); a state is (q, constrained, broken, done, stack) with the stack a tuple of symbols, the bottom first."""
import numpy as np

import dfa_ref
import heal_ref

DEAD = dfa_ref.DEAD
PUSH, POP = 0x10, 0x20
MAX_DEPTH, STATE_WORDS, MAX_RET = 64, 5, 4096
KEEP_FREE, I64 = dfa_ref.KEEP_FREE, dfa_ref.I64
CON, BRK, DONE = dfa_ref.CON, dfa_ref.BRK, dfa_ref.DONE
FREE = (0, False, False, False, ())
BROKEN = (0, False, True, False, ())

ordinary = heal_ref.ordinary
stride = dfa_ref.stride


def table_bytes(tab):
    """uint8 [S * 769 + n_ret * 32]: the table as it lies in memory"""
    trans, ret, op, accept = tab
    return np.concatenate([np.ascontiguousarray(trans, dtype="<u2").view(np.uint8).reshape(-1),
                           np.ascontiguousarray(np.asarray(ret).reshape(-1, 16), dtype="<u2").view(np.uint8).reshape(-1),
                           np.ascontiguousarray(op, dtype=np.uint8).reshape(-1), np.ascontiguousarray(accept, dtype=np.uint8)])


def from_dfa(tab):
    """the nest table of a (trans, accept): every op zero, no ret row"""
    trans, accept = tab
    return (np.asarray(trans), np.zeros((0, 16), dtype=np.uint16), np.zeros(np.asarray(trans).shape, dtype=np.uint8), np.asarray(accept))


def n_states(tab):
    return len(tab[3])


def n_ret(tab):
    return len(np.asarray(tab[1]).reshape(-1, 16))


def byte(tab, q, stack, x, max_depth):
    """One byte from (q, stack): (q', stack') or None for DEAD."""
    trans, ret, op, _ = tab
    S, v, o = n_states(tab), int(trans[q][x]), int(op[q][x])
    if o == 0:
        return (v, stack) if v < S else None
    if o & 0xF0 == PUSH:
        return (v, stack + (o & 15,)) if v < S and len(stack) < max_depth else None
    if o == POP:
        if not stack or v >= n_ret(tab):
            return None
        r = int(np.asarray(ret).reshape(-1, 16)[v][stack[-1]])
        return (r, stack[:-1]) if r < S else None
    return None


def walk(tab, q, stack, data, max_depth):
    at = (q, tuple(stack))
    for x in data:
        at = byte(tab, at[0], at[1], x, max_depth)
        if at is None:
            return None
    return at


def touches(tab, q, data):
    """The walk WITHOUT the stack: "dead", "free" (it ends alive and met no op) or "touch" (it met a byte with op != 0 first)."""
    trans, _, op, _ = tab
    for x in data:
        if int(op[q][x]):
            return "touch"
        q = int(trans[q][x])
        if q >= n_states(tab):
            return "dead"
    return "free"


def ends(tab, state):
    return bool(tab[3][state[0]]) and not state[4]


def begin(start, stack=()):
    return (int(start), True, False, False, tuple(stack))


def load(tab, state, max_depth):
    """The state as a call reads it: the regex guide's word 0; a constrained row deeper than max_depth is broken."""
    q, con, broken, done, stack = state
    if broken:
        return BROKEN
    if done:
        return (q, False, False, True, ())
    if con:
        return (q, True, False, False, tuple(stack)) if q < n_states(tab) and len(stack) <= max_depth else BROKEN
    return FREE


def allowed(toks, tab, state, end_ids=(), max_depth=MAX_DEPTH):
    """The ids a constrained configuration may draw (before the rule "never all zero"): by brute force over every ordinary id."""
    ok = {i for i, b in toks if walk(tab, state[0], state[4], b, max_depth) is not None}
    if ends(tab, state):
        ok |= set(end_ids)
    return ok


def settle(toks, tab, state, end_ids=(), max_depth=MAX_DEPTH):
    if state[1] and not allowed(toks, tab, state, end_ids, max_depth):
        return BROKEN
    return state


def mask(toks, tab, state, n_words, end_ids=(), max_depth=MAX_DEPTH):
    ok = allowed(toks, tab, state, end_ids, max_depth) if state[1] else set()
    if not ok:
        return np.full(n_words, 0xFFFFFFFF, dtype=np.uint32)
    row = np.zeros(n_words, dtype=np.uint32)
    for i in ok:
        row[i >> 5] |= np.uint32(1 << (i & 31))
    return row


def step(toks, tab, state, ids, end_ids=(), max_depth=MAX_DEPTH):
    """The loaded state after the ids, each recomputed from the rule (not settled)."""
    q, con, broken, done, stack = state
    for t in ids:
        if not con:
            break
        b = heal_ref._bytes_of(toks, t)
        at = walk(tab, q, stack, b, max_depth) if b is not None else None
        if at is not None:
            q, stack = at
            continue
        con = False
        if t in end_ids and ends(tab, (q, True, False, False, stack)):
            done, stack = True, ()
        else:
            q, broken, stack = 0, True, ()
    return (q, con, broken, done, stack)


def call(toks, tab, state, ids, n_words, end_ids=(), max_depth=MAX_DEPTH):
    """What one call does to a state row as it lies in memory -> (state written back, mask row)."""
    s = settle(toks, tab, step(toks, tab, load(tab, state, max_depth), ids, end_ids, max_depth), end_ids, max_depth)
    return s, mask(toks, tab, s, n_words, end_ids, max_depth)


def state_row(state):
    """The canonical five words of a state."""
    q, con, broken, done, stack = state
    row = [0] * STATE_WORDS
    if broken:
        row[0] = BRK
    elif done:
        row[0] = q | DONE
    elif con:
        row[0] = q | CON | len(stack) << 24
        for i, y in enumerate(stack):
            row[1 + i // 16] |= (y & 15) << (4 * (i % 16))
    return row


def raw_row(q=0, con=False, broken=False, done=False, depth=0, nibbles=(), extra=0):
    """Five words as a caller may write them, canonical or not: nibbles[i] is level i, whatever the depth says."""
    row = [(q & 0xFFFF) | (CON if con else 0) | (BRK if broken else 0) | (DONE if done else 0) | (depth & 0x7F) << 24 | extra, 0, 0, 0, 0]
    for i, y in enumerate(nibbles):
        row[1 + i // 16] |= (y & 15) << (4 * (i % 16))
    return row


def row_state(row):
    """The state a raw row stands for (nibbles at and above the depth are not part of it)."""
    w = int(row[0])
    depth = (w >> 24) & 0x7F
    stack = tuple((int(row[1 + i // 16]) >> (4 * (i % 16))) & 15 for i in range(min(depth, 64)))
    if depth > 64:
        stack = stack + (0,) * (depth - 64)                                    # (deeper than any max_depth: broken on load)
    return (w & 0xFFFF, bool(w & CON), bool(w & BRK), bool(w & DONE), stack)


def index(toks, tab, n_words):
    """(rows uint32 [S, stride], some uint8 [S], dep: a list of ascending ids per state)"""
    S = n_states(tab)
    rows = np.zeros((S, stride(n_words)), dtype=np.uint32)
    dep = [[] for _ in range(S)]
    for q in range(S):
        for i, b in toks:
            k = touches(tab, q, b)
            if k == "free":
                rows[q, i >> 5] |= np.uint32(1 << (i & 31))
            elif k == "touch":
                dep[q].append(i)
        dep[q].sort()
    return rows, (rows != 0).any(axis=1).astype(np.uint8), dep
