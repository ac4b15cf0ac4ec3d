"""Draft verification, the DEFINITION (include/splintr_hip.h, spl_dfa_draft_device / spl_nest_draft_device) by brute force: for every
node the path is built in Python and handed to the reference STEP of tests/dfa_ref.py / tests/nest_ref.py -- nothing is carried from one
node to the next.  Orphans, absent nodes and ok are stated directly.

A draft of one sequence is (ids, parent, n): ids a list of K values, parent None (a chain) or a list of K integers, n the clamped length.
`kind` is "dfa" (tab = (trans, accept), a state is a 4-tuple) or "nest" (tab = (trans, ret, op, accept), a state is a 5-tuple)."""
import dfa_ref
import nest_ref

MAX_NODES = 64
PARENT_PER_SEQ = 1


def clamp(length, K):
    """the step's clamp of d_len: None is all"""
    return K if length is None else max(0, min(int(length), K))


def parent_of(parent, i):
    return i - 1 if parent is None else int(parent[i])


def kind_of(parent, i, n):
    """"absent": at or beyond the clamped length.  "orphan": its parent is neither -1 nor an index below it, or its parent is an orphan
    or absent.  "node" otherwise."""
    if i >= n:
        return "absent"
    p = parent_of(parent, i)
    if p == -1:
        return "node"
    if not 0 <= p < i:
        return "orphan"
    return "node" if kind_of(parent, p, n) == "node" else "orphan"


def path(parent, i):
    """the nodes from the root down to node i (a node that is no orphan)"""
    p = parent_of(parent, i)
    return ([] if p == -1 else path(parent, p)) + [i]


def _ref(kind):
    return dfa_ref if kind == "dfa" else nest_ref


def _call(kind, toks, tab, state, fed, n_words, end_ids, max_depth):
    if kind == "dfa":
        return dfa_ref.call(toks, tab, state, fed, n_words, end_ids)
    return nest_ref.call(toks, tab, state, fed, n_words, end_ids, max_depth)


def _load(kind, tab, state, max_depth):
    return dfa_ref.load(tab, state) if kind == "dfa" else nest_ref.load(tab, state, max_depth)


def _step(kind, toks, tab, state, fed, end_ids, max_depth):
    if kind == "dfa":
        return dfa_ref.step(toks, tab, state, fed, end_ids)
    return nest_ref.step(toks, tab, state, fed, end_ids, max_depth)


def ok_of(kind, toks, tab, state, fed, end_ids, max_depth=64):
    """1 iff the sequence is free on input, or every id of the path was read and accepted: the sequence stayed constrained, or became
    done at the path's LAST id."""
    s = _load(kind, tab, state, max_depth)
    if not (s[1] or s[2] or s[3]):
        return 1
    for k, t in enumerate(fed):
        if not s[1]:
            return 0                                                  # (this id is not read: done or broken in front of it)
        s = _step(kind, toks, tab, s, [t], end_ids, max_depth)
        if not (s[1] or (s[3] and k == len(fed) - 1)):
            return 0
    return 1


def draft(kind, toks, tab, state, ids, parent, n_words, end_ids, max_depth=64, length=None):
    """One sequence -> (rows, ok): rows[r] = (state written, mask row) for r = 0 (the root) .. K, ok a list of K.  An absent or orphan
    node: a broken state, a row of ones, ok 0."""
    ref = _ref(kind)
    K = len(ids)
    n = clamp(length, K)
    rows = [_call(kind, toks, tab, state, [], n_words, end_ids, max_depth)]
    ok = []
    for i in range(K):
        if kind_of(parent, i, n) != "node":
            rows.append((ref.BROKEN, ref.mask(toks, tab, ref.BROKEN, n_words, end_ids)))
            ok.append(0)
            continue
        fed = [ids[j] for j in path(parent, i)]
        rows.append(_call(kind, toks, tab, state, fed, n_words, end_ids, max_depth))
        ok.append(ok_of(kind, toks, tab, state, fed, end_ids, max_depth))
    return rows, ok
