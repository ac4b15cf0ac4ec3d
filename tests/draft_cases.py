"""Drafts, trees and CHECKS shared by tests/test_draft_cpu.py (the host simulation) and tests/test_gpu_draft.py (the kernels).  Every
check takes

    draft(kind, table, n_states, n_ret, ids=, state=, parent=, lengths=, flags=, end_ids=, n_words=, max_depth=, mask_init=,
          want_live=, want_state=) -> dict(mask [B, 1 + K, n_words], ok [B, K], live [B, 1 + K] | None, state | None)

-- one draft call of the code under test, kind "dfa" or "nest", over the vocabulary `name` given to make(name) -- and the anchor also

    step(kind, table, n_states, n_ret, ids=, state=, lengths=, end_ids=, n_words=, max_depth=) -> dict(state, mask, live)

-- one STEP call of the code under test.  Results are compared with the definition of tests/draft_ref.py: mask rows, ok, live and state
rows bit for bit.  `table` is the table's bytes as they lie in memory.  The shapes are the smallest that can go wrong."""
import random

import numpy as np

import dfa_cases
import dfa_ref
import draft_ref as ref
import heal_cases
import nest_cases
import nest_ref

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
ROW_LENS = (0, 1, 2, 63, 64)


# ---------------------------------------------------------------------------------------------- helpers
def _r(kind):
    return dfa_ref if kind == "dfa" else nest_ref


def table_bytes(kind, tab):
    return dfa_ref.table_bytes(*tab) if kind == "dfa" else nest_ref.table_bytes(tab)


def shape_of(kind, tab):
    return (dfa_ref.n_states(tab), 0) if kind == "dfa" else (nest_ref.n_states(tab), nest_ref.n_ret(tab))


def raw_of(kind, states):
    return dfa_cases.words(states) if kind == "dfa" else nest_cases.rows_of(states)


def state_row(kind, s):
    return [dfa_ref.state_row(s)] if kind == "dfa" else nest_ref.state_row(s)


def vocab(name):
    return nest_cases.vocab(name)


def expect(draft, kind, toks, tab, raw, states, ids, parent, n_words, end_ids, max_depth=64, lengths=None, **kw):
    """One draft call over `states` (as the rows `raw`), ids [B, K] and parent (None, [K] or [B, K]): every row of every sequence is the
    definition's.  Returns (the call's result, per sequence (rows, ok) of the definition)."""
    B = len(states)
    ids_a = ids if isinstance(ids, np.ndarray) else np.array(ids, dtype=np.uint32).reshape(B, -1).view(np.int32)
    K = ids_a.shape[1]
    par = None if parent is None else np.asarray(parent, dtype=np.int64)
    S, R = shape_of(kind, tab)
    r = draft(kind, table_bytes(kind, tab), S, R, ids=ids_a, state=raw, parent=None if par is None else par.astype(np.int32), lengths=lengths, end_ids=end_ids,
              n_words=n_words, max_depth=max_depth, **kw)
    assert r["mask"].shape == (B, 1 + K, n_words) and r["ok"].shape == (B, K)
    wants = []
    for b, st in enumerate(states):
        fed = [int(x) & 0xFFFFFFFF if ids_a.dtype != np.int64 else int(x) for x in ids_a[b]]
        p = None if par is None else (par[b] if par.ndim == 2 else par).tolist()
        rows, ok = ref.draft(kind, toks, tab, st, fed, p, n_words, end_ids, max_depth, None if lengths is None else int(lengths[b]))
        assert r["ok"][b].tolist() == ok, (b, st, fed, p, r["ok"][b].tolist(), ok)
        for k, (want, row) in enumerate(rows):
            assert r["mask"][b, k].tolist() == row.tolist(), (b, k, st, fed, p)
            if r["live"] is not None:
                assert int(r["live"][b, k]) == int(want[1]), (b, k, st, fed, p)
            if r["state"] is not None:
                assert [int(x) for x in np.atleast_1d(r["state"][b, k])] == state_row(kind, want), (b, k, st, fed, p, want)
        wants.append((rows, ok))
    return r, wants


# ---------------------------------------------------------------------------------------------- trees
def chain(K):
    return [i - 1 for i in range(K)]


def star(K):
    return [-1] * K


def binary(K):
    """a complete binary tree: node 0 below the root, nodes 2i + 1 and 2i + 2 below node i"""
    return [(i - 1) // 2 if i else -1 for i in range(K)]


def caterpillar(K):
    """a spine of the even nodes, a leaf on every one of them"""
    return [-1 if i == 0 else (i - 1 if i % 2 else i - 2) for i in range(K)]


def random_tree(K, rng):
    return [rng.randrange(-1, i) for i in range(K)]


TREES = {"chain": chain, "star": star, "binary": binary, "caterpillar": caterpillar}


def fill_ids(kind, toks, tab, state, parent, K, end_ids, rng, pool, p_bad=0.12, max_depth=64):
    """Ids for the nodes of a tree: the id of a node is drawn from what the definition allows behind its parent -- one that leaves
    something to draw, where there is one -- or, with probability p_bad and wherever the parent is no longer constrained, from `pool`."""
    R = _r(kind)
    extra = () if kind == "dfa" else (max_depth,)
    load = R.load(tab, state, *extra)
    after, ids = {}, []
    forever = set(range(len(tab[-1])))                                 # the states an endless run of ordinary ids can start in (without the stack)
    while kind == "dfa":
        keep = {q for q in forever if any(dfa_ref.walk(tab, q, b) in forever for _, b in toks)}
        if keep == forever:
            break
        forever = keep
    for i in range(K):
        p = parent[i] if parent is not None else i - 1
        at = load if p == -1 else after.get(p)
        t = rng.choice(pool)
        if at is not None and at[1] and rng.random() >= p_bad:
            ok = sorted(R.allowed(toks, tab, at, end_ids, *extra))
            on = [x for x in ok if x not in end_ids and (lambda s: s[1] and s[0] in forever and R.allowed(toks, tab, s, (), *extra))(R.step(toks, tab, at, [x], end_ids, *extra))]
            if on or ok:
                t = rng.choice(on or ok)
        ids.append(t)
        after[i] = R.step(toks, tab, at, [t], end_ids, *extra) if at is not None else None
    return ids


class Case:
    """a vocabulary, a table of each kind over it, END ids and probe ids"""

    def __init__(self, name):
        self.name = name
        self.vocab, self.specials, self.toks = vocab(name)
        self.nw = nest_cases.min_words(self.vocab)
        self.pool = heal_cases.probe_ids(self.vocab, self.specials)
        if name in dfa_cases.TOYS:
            self.sp, self.od, self.last = dfa_cases.special_ids(name)
            self.dfa = dfa_cases.compiled(dfa_cases.PROBE_PATTERNS[name])
            self.end = (self.sp, self.last)
        elif name == "brackets":
            self.nest, self.end = nest_cases.brackets_table(), (25, 40)
        elif name == "paren":
            self.nest, self.end = nest_cases.paren_table(), (9,)

    def tab(self, kind):
        return self.dfa if kind == "dfa" else (self.nest if hasattr(self, "nest") else nest_ref.from_dfa(self.dfa))

    def starts(self, kind, n):
        """n constrained states spread over the table's states (nest: with stacks of a few depths over a bracket table)"""
        tab = self.tab(kind)
        S = shape_of(kind, tab)[0]
        if kind == "dfa":
            return [dfa_ref.begin(b % S) for b in range(n)]
        if self.name == "brackets":
            return [nest_ref.begin(b % S, tuple(1 + (b + j) % 2 for j in range((0, 1, 3, 16)[b % 4]))) for b in range(n)]
        return [nest_ref.begin(b % S) for b in range(n)]


# ---------------------------------------------------------------------------------------------- checks
def check_anchor(draft, step, name, kinds=("dfa", "nest")):
    """THE ANCHOR.  With no parents, row 1 + i equals a STEP call of the code under test with lengths i + 1, for every i, and row 0 the
    step at row_len 0 -- for the regex guide and for the nest guide; and the nest draft over the ops-zero table equals the regex draft bit
    for bit."""
    c = Case(name)
    rng = random.Random(5)
    K, B = 5, 6
    for kind in kinds:
        tab = c.tab(kind)
        S, R = shape_of(kind, tab)
        states = c.starts(kind, B - 1) + [_r(kind).FREE]
        ids = np.array([fill_ids(kind, c.toks, tab, s, None, K, c.end, rng, c.pool, p_bad=0.2) for s in states], dtype=np.uint32).view(np.int32)
        raw = raw_of(kind, states)
        d = draft(kind, table_bytes(kind, tab), S, R, ids=ids, state=raw, parent=None, end_ids=c.end, n_words=c.nw, max_depth=64)
        for i in range(-1, K):
            s = step(kind, table_bytes(kind, tab), S, R, ids=ids if i >= 0 else ids[:, :0], state=raw, lengths=None if i < 0 else np.full(B, i + 1, dtype=np.int32),
                     end_ids=c.end, n_words=c.nw, max_depth=64)
            assert (d["mask"][:, 1 + i] == s["mask"]).all(), (kind, i)
            assert (d["live"][:, 1 + i] == s["live"]).all(), (kind, i)
            assert (np.asarray(d["state"][:, 1 + i]).reshape(B, -1) == np.asarray(s["state"]).reshape(B, -1)).all(), (kind, i)
        assert (np.diff(d["ok"].astype(np.int8), axis=1) <= 0).all(), "ok is monotone along a chain"
        if kind == "dfa":
            first = (d, ids)
        elif "dfa" in kinds:                                           # the ops-zero table, fed the regex guide's ids
            ids0 = first[1]
            z = draft("nest", table_bytes("nest", tab), S, R, ids=ids0, state=nest_cases.rows_of([s + ((),) for s in c.starts("dfa", B - 1)] + [nest_ref.FREE]),
                      parent=None, end_ids=c.end, n_words=c.nw, max_depth=64)
            assert (z["mask"] == first[0]["mask"]).all() and (z["ok"] == first[0]["ok"]).all() and (z["live"] == first[0]["live"]).all()
            assert (z["state"][:, :, 0] == first[0]["state"]).all() and (z["state"][:, :, 1:] == 0).all()


def check_topologies(draft, name, kinds=("dfa", "nest"), row_lens=ROW_LENS):
    """A chain given explicitly, a star, a complete binary tree, a caterpillar (at 64 nodes: a chain of depth 64 among them) and random
    topological trees at 0, 1, 2, 63 and 64 nodes, their ids mostly acceptable, some not; one shared row of parents against the same row
    repeated per sequence."""
    c = Case(name)
    rng = random.Random(17)
    full = 0
    for kind in kinds:
        tab = c.tab(kind)
        B = 3
        states = c.starts(kind, B)
        raw = raw_of(kind, states)
        for K in row_lens:
            trees = [f(K) for f in TREES.values()] + [random_tree(K, rng) for _ in range(2)]
            for t_i, tree in enumerate(trees):
                ids = [fill_ids(kind, c.toks, tab, s, tree, K, c.end, rng, c.pool, p_bad=0.0 if (t_i, b) == (0, 0) else (0.04 if K > 8 else 0.25))
                       for b, s in enumerate(states)]                  # (the first sequence's chain is acceptable whole: depth 64)
                r, wants = expect(draft, kind, c.toks, tab, raw, states, ids, tree, c.nw, c.end)
                if t_i == 0:
                    r2, _ = expect(draft, kind, c.toks, tab, raw, states, ids, None, c.nw, c.end)       # the chain, given and implied
                    assert all((r[k] == r2[k]).all() for k in ("mask", "ok", "live", "state"))
                    full += int(K == 64 and any(sum(ok) == 64 for _, ok in wants))
                rp, _ = expect(draft, kind, c.toks, tab, raw, states, ids, [tree] * B, c.nw, c.end)    # one row for all | a row per sequence
                assert all((r[k] == rp[k]).all() for k in ("mask", "ok", "live", "state"))
            if K >= 2:                                                 # per sequence, different trees
                per = [random_tree(K, rng) for _ in range(B)]
                ids = [fill_ids(kind, c.toks, tab, s, per[b], K, c.end, rng, c.pool) for b, s in enumerate(states)]
                expect(draft, kind, c.toks, tab, raw, states, ids, per, c.nw, c.end)
    if 64 in row_lens:
        assert full, "no chain of depth 64 was accepted whole"


def check_order(draft, name="gaps", kind="dfa"):
    """NAMED CHECK (the mutant "order": the ancestors walked in descending order must fail here).  Paths of two and more ids, every id
    acceptable where it stands: ok is 1 everywhere, and the state behind a path is the one its ids lead to in root-to-node order."""
    c = Case(name)
    rng = random.Random(3)
    tab = c.tab(kind)
    states = c.starts(kind, 4)
    seen = 0
    for tree in (chain(6), binary(7), caterpillar(8), random_tree(9, rng)):
        ids = [fill_ids(kind, c.toks, tab, s, tree, len(tree), (), rng, c.pool, p_bad=0.0) for s in states]      # (no END id: that is check_done_child's)
        keep = [b for b, s in enumerate(states) if all(ref.draft(kind, c.toks, tab, s, ids[b], tree, c.nw, c.end)[1])]  # (no rejected id: check_rejected's)
        assert len(keep) >= 2
        sts = [states[b] for b in keep]
        r, wants = expect(draft, kind, c.toks, tab, raw_of(kind, sts), sts, [ids[b] for b in keep], tree, c.nw, c.end)
        seen += sum(sum(ok) for _, ok in wants)
    assert seen > 40


def check_rejected(draft, name="gaps", kind="dfa"):
    """NAMED CHECK (the mutant "ok": ok that ignores a rejected ancestor must fail here).  A rejected id at node 0, in the middle and at the
    last node of a chain, and with children in a tree: the node and everything below it has ok 0 and a row of ones; its siblings do not
    care.  The rejected ids: one whose walk dies, a special that is no END id, an id of neither map, an int64 value outside 32 bits."""
    c = Case(name)
    rng = random.Random(8)
    tab = c.tab(kind)
    R = _r(kind)
    s0 = c.starts(kind, 1)[0]
    K = 5
    good = fill_ids(kind, c.toks, tab, s0, None, K, (), rng, c.pool, p_bad=0.0)
    assert ref.draft(kind, c.toks, tab, s0, good, None, c.nw, c.end)[1] == [1] * K, "the table leaves no chain of five"
    dead = next(t for t in sorted(c.vocab) if t not in R.allowed(c.toks, tab, R.load(tab, s0, *(() if kind == "dfa" else (64,))), c.end))
    top = max(max(c.vocab), max(c.specials or [0]))
    not_end = [t for t in sorted(c.specials) if t not in c.end][:1]            # a special that is no END id, where the vocabulary has one
    for bad in [dead] + not_end + [top + 7, 0xFFFFFFFF]:
        for at in (0, 2, K - 1):
            ids = list(good)
            ids[at] = bad
            _, wants = expect(draft, kind, c.toks, tab, raw_of(kind, [s0]), [s0], [ids], None, c.nw, c.end)
            if bad != dead or at == 0:
                assert wants[0][1] == [1] * at + [0] * (K - at), (bad, at, wants[0][1])
    wide = np.array([good[:2] + [(1 << 32) + good[2]] + good[3:]], dtype=np.int64)
    _, wants = expect(draft, kind, c.toks, tab, raw_of(kind, [s0]), [s0], wide, None, c.nw, c.end)
    assert wants[0][1] == [1, 1, 0, 0, 0]
    # a tree: node 1 is rejected; its children 3 and 4 and grandchild 5 fall with it, its sibling 2 and 2's child 6 stand
    tree = [-1, 0, 0, 1, 1, 3, 2]
    ids = fill_ids(kind, c.toks, tab, s0, tree, 7, (), rng, c.pool, p_bad=0.0)
    ids[1] = top + 7
    _, wants = expect(draft, kind, c.toks, tab, raw_of(kind, [s0]), [s0], [ids], tree, c.nw, c.end)
    assert wants[0][1] == [1, 0, 1, 0, 0, 0, 1], wants[0][1]
    assert all(wants[0][0][1 + i][0] == R.BROKEN for i in (1, 3, 4, 5))


def check_done_child(draft, name="gaps", kind="dfa"):
    """NAMED CHECK (the mutant "done": a child of a node that ended the sequence accepted must fail here).  An END id in an accepting state
    with a child under it: the node is ok and done, the child is not ok and its row is the done row; an END id in a state that does not
    accept: rejected; an END id that is ordinary and walks on: an ordinary id, its child stands."""
    c = Case(name)
    tab = c.tab(kind)
    R = _r(kind)
    extra = () if kind == "dfa" else (64,)
    S = shape_of(kind, tab)[0]
    accepting = [R.begin(q) for q in range(S) if tab[-1][q] and R.allowed(c.toks, tab, R.begin(q), (), *extra)]
    plain = [R.begin(q) for q in range(S) if not tab[-1][q]]
    assert accepting and plain
    sa, sn = accepting[0], plain[0]
    on = next(t for t in sorted(R.allowed(c.toks, tab, sa, (), *extra)) if R.allowed(c.toks, tab, R.step(c.toks, tab, sa, [t], (), *extra), (), *extra))
    end = c.end
    # node 0: END behind an accepting state; node 1 below it; node 2 a sibling that walks on; node 3 below node 2
    ids = [end[0], on, on, end[0]]
    tree = [-1, 0, -1, 2]
    r, wants = expect(draft, kind, c.toks, tab, raw_of(kind, [sa]), [sa], [ids], tree, c.nw, end)
    rows, ok = wants[0]
    assert ok[0] == 1 and ok[1] == 0 and ok[2] == 1 and rows[1][0][3] and rows[2][0][3] and rows[1][0] == rows[2][0], (ok, rows[1][0], rows[2][0])
    _, early = expect(draft, kind, c.toks, tab, raw_of(kind, [sn]), [sn], [[end[0], end[-1]]], star(2), c.nw, end)      # END too early (no child: that is check_rejected's)
    assert early[0][1] == [0, 0] and early[0][0][1][0] == R.BROKEN
    assert (r["mask"][0, 1] == 0xFFFFFFFF).all() and (r["mask"][0, 2] == 0xFFFFFFFF).all()
    # a chain END, END: the second is not read
    _, wants = expect(draft, kind, c.toks, tab, raw_of(kind, [sa]), [sa], [[end[0], end[0], on]], None, c.nw, end)
    assert wants[0][1] == [1, 0, 0]
    # an END id that is ordinary and walks on is an ordinary id
    _, wants = expect(draft, kind, c.toks, tab, raw_of(kind, [sa]), [sa], [[on, on]], None, c.nw, (on,) + end)
    assert wants[0][1][0] == 1 and wants[0][0][1][0][1], wants[0]


def check_orphans(draft, name="gaps", kind="dfa"):
    """Parents i, i + 1, -2, INT32_MIN and INT32_MAX; a valid child of an orphan; a child of an absent node; a cycle-looking pair: ok 0,
    live 0, a broken row, ones -- and the sound nodes beside them are what they are without them."""
    c = Case(name)
    rng = random.Random(21)
    tab = c.tab(kind)
    R = _r(kind)
    s0 = c.starts(kind, 2)
    K = 8
    for bad in (None, "self", "next", -2, I32_MIN, I32_MAX, K, 63, 64):
        tree = [-1, 0, 1, 2, 3, -1, 5, 5]
        if bad is not None:
            tree[2] = 2 if bad == "self" else (3 if bad == "next" else bad)          # node 2 is an orphan; 3 and 4 hang below it
        ids = [fill_ids(kind, c.toks, tab, s, [-1, 0, 1, 2, 3, -1, 5, 5], K, (), rng, c.pool, p_bad=0.0) for s in s0]
        r, wants = expect(draft, kind, c.toks, tab, raw_of(kind, s0), s0, ids, tree, c.nw, c.end)
        for b in range(2):
            rows, ok = wants[b]
            if bad is not None:
                assert ok[2:5] == [0, 0, 0] and all(rows[1 + i][0] == R.BROKEN for i in (2, 3, 4)), (bad, ok)
                assert (r["mask"][b, 3:6] == 0xFFFFFFFF).all() and (r["live"][b, 3:6] == 0).all()
            assert ok[0] == ok[1] == ok[5] == 1
    # a child of an absent node, and a per-sequence row of parents with an orphan in one sequence only
    tree = [-1, 0, 1, 2, -1, 4]
    ids = [fill_ids(kind, c.toks, tab, s, tree, 6, (), rng, c.pool, p_bad=0.0) for s in s0]
    for n in (0, 1, 2, 5, 6):
        _, wants = expect(draft, kind, c.toks, tab, raw_of(kind, s0), s0, ids, tree, c.nw, c.end, lengths=np.array([n, 6], dtype=np.int32))
        assert wants[0][1] == [int(i < n) for i in range(6)] and wants[1][1] == [1] * 6
    per = [tree, [-1, 0, 7, 2, -1, 4]]
    _, wants = expect(draft, kind, c.toks, tab, raw_of(kind, s0), s0, ids, per, c.nw, c.end)
    assert wants[0][1] == [1] * 6 and wants[1][1] == [1, 1, 0, 0, 1, 1]


def check_lengths(draft, name="gaps", kind="dfa", chains=True):
    """d_len negative, 0, below, at and above row_len, for a chain and for a star (paths of one id: the walk's order cannot matter)."""
    c = Case(name)
    rng = random.Random(4)
    tab = c.tab(kind)
    K = 4
    lens = np.array([-3, 0, 1, K - 1, K, K + 5, I32_MAX, I32_MIN], dtype=np.int32)
    states = c.starts(kind, len(lens))
    for tree in ((None, star(K)) if chains else (star(K),)):
        ids = [fill_ids(kind, c.toks, tab, s, tree, K, (), rng, c.pool, p_bad=0.0) for s in states]
        _, wants = expect(draft, kind, c.toks, tab, raw_of(kind, states), states, ids, tree, c.nw, c.end, lengths=lens)
        for b, n in enumerate([0, 0, 1, K - 1, K, K, K, 0]):
            assert wants[b][1][n:] == [0] * (K - n)
            assert all(rows[0] == _r(kind).BROKEN for rows in wants[b][0][1 + n:])


def check_input_states(draft, name="gaps"):
    """Free, done, broken and q >= n_states on input, with the ok rows that follow: free 1 everywhere (nothing is read, rows of ones),
    the others 0; words no call writes; int32 and int64 ids; every probe id as a single node from every state."""
    c = Case(name)
    tab = c.tab("dfa")
    S = dfa_ref.n_states(tab)
    raw = [dfa_ref.raw_row(0), dfa_ref.raw_row(1, done=True), dfa_ref.raw_row(2, broken=True), dfa_ref.raw_row(S, con=True), dfa_ref.raw_row(0xFFFF, con=True),
           dfa_ref.raw_row(1, con=True, done=True), dfa_ref.raw_row(0, con=True), dfa_ref.raw_row(1, con=True, extra=1 << 40)]
    states = [dfa_ref.row_state(x) for x in raw]
    ids = [[0, 0, c.sp]] * len(raw)
    for parent in (None, star(3), [-1, 0, 0]):
        for dtype in (np.int32, np.int64):
            r, wants = expect(draft, "dfa", c.toks, tab, np.array(raw, dtype=np.uint64), states, np.array(ids, dtype=dtype), parent, c.nw, c.end)
            assert wants[0][1] == [1, 1, 1] and all(w[1] == [0, 0, 0] for w in wants[1:6])
            assert (r["mask"][:6] == 0xFFFFFFFF).all() and (r["live"][:6] == 0).all()
            assert [int(r["state"][b, 0]) for b in range(6)] == [0, 1 | dfa_ref.DONE, dfa_ref.BRK, dfa_ref.BRK, dfa_ref.BRK, 1 | dfa_ref.DONE]
    pairs = [(dfa_ref.begin(q), t) for q in range(S) for t in c.pool + [c.last]]
    expect(draft, "dfa", c.toks, tab, dfa_cases.words([s for s, _ in pairs]), [s for s, _ in pairs], [[t] for _, t in pairs], None, c.nw, (c.sp, c.od, c.last))
    # the nest rows: a depth above max_depth, garbage nibbles above the depth, done and free rows with a depth
    cb = Case("brackets")
    raw = [nest_ref.raw_row(0, con=True, depth=2, nibbles=(1, 2, 9, 9, 15) + (7,) * 59), nest_ref.raw_row(0, con=True, depth=0, nibbles=(3,) * 64),
           nest_ref.raw_row(1, con=True, depth=16, nibbles=(1,) * 16 + (5,) * 48), nest_ref.raw_row(0, con=True, depth=17, nibbles=(2,) * 17 + (6,)),
           nest_ref.raw_row(0, con=True, depth=65, nibbles=(1,) * 64), nest_ref.raw_row(0, done=True, depth=5, nibbles=(1,) * 5),
           nest_ref.raw_row(0, depth=5, nibbles=(1,) * 5), nest_ref.raw_row(2, con=True, depth=1, nibbles=(1,))]
    states = [nest_ref.row_state(x) for x in raw]
    for max_depth in (64, 8):
        _, wants = expect(draft, "nest", cb.toks, cb.nest, np.array(raw, dtype=np.uint64), states, [[2, 0, 4]] * len(raw), [-1, 0, -1], cb.nw, cb.end,
                          max_depth=max_depth)
        assert wants[0][1] == [0, 0, 1] and wants[4][1] == [0, 0, 0] and wants[5][1] == [0, 0, 0] and wants[6][1] == [1, 1, 1] and wants[7][1] == [0, 0, 0]
        assert (wants[2][1] == [0, 0, 0]) == (max_depth == 8)


def check_stack(draft):
    """The nest guide's stack along paths: input stacks of depth 0, 1, 15, 16, 17, 63 and 64 with max_depth 64 and max_depth equal to the
    depth; max_depth 1; a path whose ids push past max_depth; a token that pops three levels with two on the stack; ids that push and pop
    inside themselves; sibling paths that leave different stacks behind one parent."""
    c = Case("brackets")
    tab = c.nest
    rng = random.Random(2)
    popped3 = over = 0
    tree = [-1, 0, 0, 1, 1, 2, -1, 6]
    for depth in (0, 1, 15, 16, 17, 63, 64):
        stack = tuple(rng.choice((1, 2)) for _ in range(depth))
        for max_depth in sorted({64, max(depth, 1)}):
            states = [nest_ref.begin(q, stack) for q in (0, 1)]
            for _ in range(2):
                ids = [fill_ids("nest", c.toks, tab, s, tree, len(tree), c.end, rng, c.pool, p_bad=0.2, max_depth=max_depth) for s in states]
                expect(draft, "nest", c.toks, tab, nest_cases.rows_of(states), states, ids, tree, c.nw, c.end, max_depth=max_depth)
    # ")))" with two levels: dead; "))" then ")" from three levels: alive to depth 0; pushes past max_depth 3 along a path
    by = {b: t for t, b in c.vocab.items()}
    s = nest_ref.begin(0, (1, 1))
    _, wants = expect(draft, "nest", c.toks, tab, nest_cases.rows_of([s]), [s], [[by[b")))"], by[b"))"], by[b")"], by[b"a"]]], [-1, -1, 1, 1], c.nw, c.end)
    assert wants[0][1] == [0, 1, 0, 1] and wants[0][0][2][0] == (0, True, False, False, ())
    popped3 += 1
    s = nest_ref.begin(0, (1,))
    ids = [by[b"(("], by[b"("], by[b"a"], by[b"(a)"], by[b")"]]
    for max_depth in (3, 4, 1):
        _, wants = expect(draft, "nest", c.toks, tab, nest_cases.rows_of([s]), [s], [ids], [-1, 0, 0, 2, 1], c.nw, c.end, max_depth=max_depth)
        assert wants[0][1] == {3: [1, 0, 1, 0, 0], 4: [1, 1, 1, 1, 1], 1: [0, 0, 0, 0, 0]}[max_depth], (max_depth, wants[0][1])
        over += 1
    assert popped3 and over


def check_deps(draft):
    """Dependent ids on both sides of a row's piece boundary in the rows of different nodes of one sequence, dep lists of every length of
    nest_cases.DEP_LENGTHS, and the state whose every id touches the stack (nothing in its row: the settle asks the dependent ids)."""
    c = Case("deps")
    tab = nest_cases.deps_table()
    nw = c.nw + 1
    sp = 70150
    rng = random.Random(6)
    want_rows, want_some, want_dep = nest_ref.index(c.toks, tab, nw)
    assert max(max(d) for d in want_dep if d) >= 32 * 1024 and not want_some[6] and len(want_dep[6]) == 256
    stacks = [(), (1,), (3, 8), (7, 8, 1, 2)]
    states = [nest_ref.begin(q, st) for q in (0, 2, 4, 5, 6, 7) for st in stacks]
    tree = [-1, 0, -1, 2, 3]
    ids = [fill_ids("nest", c.toks, tab, s, tree, 5, (sp,), rng, c.pool, p_bad=0.1) for s in states]
    for max_depth in (4, 64):
        _, wants = expect(draft, "nest", c.toks, tab, nest_cases.rows_of(states), states, ids, tree, nw, (sp,), max_depth=max_depth)
    six = [rows for (rows, ok), s in zip(wants, states) if s[0] == 6]
    assert any(r[0][0] == nest_ref.BROKEN for r in six) and any(r[0][0][1] for r in six)       # state 6: under (3, 8) no dependent id lives
    reached = {rows[k][0][0] for rows, _ in wants for k in range(1, 6) if rows[k][0][1]}
    assert len(reached) >= 4, reached


def check_layout_and_flags(draft, name="gaps", kinds=("dfa", "nest")):
    """KEEP_FREE over poisoned masks; rows of 4k - 1, 4k and 4k + 1 words; live and the state rows absent and given."""
    for kind in kinds:
        c = Case(name if kind == "dfa" else "brackets")
        tab = c.tab(kind)
        rng = random.Random(12)
        R = _r(kind)
        states = c.starts(kind, 3) + [R.FREE, (1, False, False, True) + (() if kind == "dfa" else ((),))]
        B, K = len(states), 3
        tree = [-1, 0, -1]
        ids = [fill_ids(kind, c.toks, tab, s, tree, K, c.end, rng, c.pool, p_bad=0.3) for s in states]
        k4 = (c.nw + 4) // 4 * 4
        for nw in sorted({c.nw, k4 - 1, k4, k4 + 1, k4 + 4}):
            end = c.end + (32 * nw - 1,)
            for want_live, want_state in ((True, True), (False, True), (True, False), (False, False)):
                expect(draft, kind, c.toks, tab, raw_of(kind, states), states, ids, tree, nw, end, want_live=want_live, want_state=want_state)
        init = (np.arange(B * (1 + K) * c.nw, dtype=np.uint32).reshape(B, 1 + K, c.nw) + 77)
        S, Rr = shape_of(kind, tab)
        r = draft(kind, table_bytes(kind, tab), S, Rr, ids=np.array(ids, dtype=np.uint32).view(np.int32), state=raw_of(kind, states), parent=np.array(tree, dtype=np.int32),
                  flags=dfa_ref.KEEP_FREE, end_ids=c.end, n_words=c.nw, max_depth=64, mask_init=init)
        kept = written = 0
        for b, st in enumerate(states):
            rows, ok = ref.draft(kind, c.toks, tab, st, ids[b], tree, c.nw, c.end)
            assert r["ok"][b].tolist() == ok
            for k, (want, row) in enumerate(rows):
                assert int(r["live"][b, k]) == int(want[1])
                assert r["mask"][b, k].tolist() == (row.tolist() if want[1] else init[b, k].tolist()), (kind, b, k)
                kept += not want[1]
                written += bool(want[1])
        assert kept and written
