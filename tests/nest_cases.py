"""Tables, states and CHECKS shared by tests/test_nest_cpu.py (the host simulation) and tests/test_gpu_nest.py (the kernels).  Every check
takes `run(table, n_states, n_ret, ids=, state=, max_depth=, lengths=, flags=, end_ids=, n_words=, in_place=, mask_init=) -> dict(state
[B, 5], mask, live)` -- one step call of the code under test over a vocabulary -- and / or `index(table, n_states, n_ret, n_words,
dep_cap=None) -> (rows, some, dep_off, dep_ids)` (dep_cap None: the exact size; one that is too small raises TooSmall(n_dep) after the
caller of the code under test saw that nothing behind the cap was written), and compares them with the definition of tests/nest_ref.py,
state rows, index words and dep entries bit for bit.  `table` is the table's bytes as they lie in memory.

dfa_run / dfa_index route the callables of tests/dfa_cases.py through the nest calls with ops-zero tables: THE ANCHOR."""
import random

import numpy as np

import dfa_cases
import dfa_ref
import heal_cases
import nest_ref as ref

NO_IDS = dfa_cases.NO_IDS
min_words = dfa_cases.min_words
bit = dfa_cases.bit
D = ref.DEAD


class TooSmall(Exception):
    """dep_cap does not hold the dependent entries: args[0] is their number"""


# ---------------------------------------------------------------------------------------------- vocabularies
def vocab_brackets():
    """a and two kinds of brackets: tokens that push, pop, do both inside themselves, pop more than one level, and mismatch"""
    toks = [b"a", b"(", b")", b"[", b"]", b"))", b"()", b"a)", b")))", b"]]", b"(]", b"[)", b"([", b")]", b"(a)", b"[]", b"[a]", b"aa", b"((", b"a(",
            b"]a", b"))]", b"(a)a", b"[[a]]"]
    vocab = dict(enumerate(toks))
    del vocab[11]                                                     # (a gap)
    vocab[37] = b"[)"
    return vocab, {25: b"<e>", 40: b")"}


def vocab_deps():
    """Every single byte as a token, the ids spread over more than 65 536 (two pieces of a row) with gaps, in no order of the bytes"""
    perm = list(range(256))
    random.Random(11).shuffle(perm)
    return {perm[x] * 275 + perm[x] % 7: bytes([x]) for x in range(256)}, {70150: b"<e>"}


def vocab_paren():
    """the toy vocabulary of the hand-worked examples (tests/test_nest_cpu.py)"""
    return {0: b"(", 1: b")", 2: b"))", 3: b"()", 4: b"a)", 5: b"a"}, {}


VOCABS = {"brackets": vocab_brackets, "deps": vocab_deps, "paren": vocab_paren}


def vocab(name):
    """(vocabulary, specials, ordinary tokens) of one of VOCABS or of the toy vocabularies of tests/dfa_cases.py"""
    v, specials = (VOCABS.get(name) or dfa_cases.TOYS[name])()
    return v, specials, ref.ordinary(v)


# ---------------------------------------------------------------------------------------------- tables
def paren_table():
    """a* ( ... ) by hand, three states: 0 -a-> 0, 0 -(-> 1 pushing 0, 1 -a-> 1, 1 -(-> 1 pushing 1, ) pops: symbol 1 returns to 1, symbol 0
    to 2.  State 0 pops too (and dies: its stack is empty).  States 1 and 2 accept -- END may follow 1 only with an empty stack, which no
    walk from the start reaches."""
    trans = np.full((3, 256), D, dtype=np.uint16)
    op = np.zeros((3, 256), dtype=np.uint8)
    trans[0, ord("a")], trans[1, ord("a")] = 0, 1
    trans[0, ord("(")], op[0, ord("(")] = 1, ref.PUSH | 0
    trans[1, ord("(")], op[1, ord("(")] = 1, ref.PUSH | 1
    trans[0, ord(")")], op[0, ord(")")] = 0, ref.POP
    trans[1, ord(")")], op[1, ord(")")] = 0, ref.POP
    ret = np.full((1, 16), D, dtype=np.uint16)
    ret[0, 0], ret[0, 1] = 2, 1
    return trans, ret, op, np.array([0, 1, 1], dtype=np.uint8)


def brackets_table():
    """Two kinds of brackets around a's: state 0 (content, accepts), state 1 (just opened: a, an opener or ")" -- "[]" is refused).  ( pushes
    1, [ pushes 2; ) pops through ret row 0, ] through ret row 1: a bracket closed by the other kind is DEAD."""
    trans = np.full((2, 256), D, dtype=np.uint16)
    op = np.zeros((2, 256), dtype=np.uint8)
    for q in (0, 1):
        trans[q, ord("a")] = 0
        trans[q, ord("(")], op[q, ord("(")] = 1, ref.PUSH | 1
        trans[q, ord("[")], op[q, ord("[")] = 1, ref.PUSH | 2
        trans[q, ord(")")], op[q, ord(")")] = 0, ref.POP
    trans[0, ord("]")], op[0, ord("]")] = 1, ref.POP
    ret = np.full((2, 16), D, dtype=np.uint16)
    ret[0, 1] = ret[1, 2] = 0
    return trans, ret, op, np.array([1, 0], dtype=np.uint8)


BAD_OPS = (0x01, 0x0F, 0x21, 0x2F, 0x30, 0x40, 0x80, 0xFF)


def random_table(n, alphabet, seed, n_ret=None, density=0.6):
    """n states over the bytes of `alphabet`: transitions as dfa_cases.random_automaton's (values at or above n must read as DEAD); a byte's
    op is 0, a push of a random symbol, a pop, or a byte that is no op; pops name ret rows inside and outside n_ret, ret values lie inside
    and outside n.  n_ret 0: every pop is DEAD."""
    rng = random.Random(seed * 104729 + n)
    trans, accept = dfa_cases.random_automaton(n, alphabet, seed, density)
    n_ret = rng.choice([1, 2, 5]) if n_ret is None else n_ret
    op = np.zeros((n, 256), dtype=np.uint8)
    junk = np.random.RandomState(seed + n).choice(np.array([0, 0, 0, 0x11, 0x20, 0x33], dtype=np.uint8), size=(n, 256))
    al = set(alphabet)
    for q in range(n):
        for x in range(256):
            if x not in al:
                op[q, x] = junk[q, x]
                continue
            r = rng.random()
            if r < 0.15:
                op[q, x] = ref.PUSH | rng.randrange(16)
            elif r < 0.30:
                op[q, x] = ref.POP
                trans[q, x] = rng.choice([0, max(0, n_ret - 1), n_ret, n_ret + 1, 0xFFFF]) if rng.random() < 0.3 else rng.randrange(max(1, n_ret))
            elif r < 0.34:
                op[q, x] = rng.choice(BAD_OPS)
    ret = np.array([[rng.randrange(n) if rng.random() < 0.75 else rng.choice([n, n + 1, 0xFFFF, 0x8000]) for _ in range(16)] for _ in range(n_ret)],
                   dtype=np.uint16).reshape(n_ret, 16)
    return trans, ret, op, accept


# ---------------------------------------------------------------------------------------------- the anchor
def dfa_run(run):
    """a `run` of tests/dfa_cases.py over the nest call: the DFA table with every op zero, the state word as word 0 of five"""
    def go(table, n_states, *, ids, state, **kw):
        table = np.asarray(table, dtype=np.uint8)
        nest = np.concatenate([table[:n_states * 512], np.zeros(n_states * 256, dtype=np.uint8), table[n_states * 512:]])
        words = np.asarray(state, dtype=np.uint64).reshape(-1)
        rows = np.zeros((len(words), ref.STATE_WORDS), dtype=np.uint64)
        rows[:, 0] = words
        r = run(nest, n_states, 0, ids=ids, state=rows, **kw)
        assert (r["state"][:, 1:] == 0).all(), "an ops-zero table left a stack"
        return dict(r, state=r["state"][:, 0].copy())
    return go


def dfa_index(index):
    """an `index` of tests/dfa_cases.py over the nest call; every dep list of an ops-zero table is empty"""
    def go(table, n_states, n_words):
        table = np.asarray(table, dtype=np.uint8)
        nest = np.concatenate([table[:n_states * 512], np.zeros(n_states * 256, dtype=np.uint8), table[n_states * 512:]])
        rows, some, dep_off, dep_ids = index(nest, n_states, 0, n_words, dep_cap=0)
        assert (np.asarray(dep_off) == 0).all() and len(dep_ids) == 0, "an ops-zero table has dependent ids"
        return rows, some
    return go


# ---------------------------------------------------------------------------------------------- checks
def rows_of(states):
    return np.array([ref.state_row(s) for s in states], dtype=np.uint64).reshape(len(states), ref.STATE_WORDS)


def expect(run, toks, tab, raw_rows, states, ids, n_words, end_ids, max_depth=64, **kw):
    """One call over `states` (as the rows raw_rows) and ids [B, K]: state rows, masks and live bytes are the definition's.  Returns (the
    call's result, the states it left)."""
    ids_a = ids if isinstance(ids, np.ndarray) else np.array(ids, dtype=np.uint32).reshape(len(states), -1).view(np.int32)
    lens = kw.get("lengths")
    r = run(ref.table_bytes(tab), ref.n_states(tab), ref.n_ret(tab), ids=ids_a, state=raw_rows, max_depth=max_depth, end_ids=end_ids, n_words=n_words, **kw)
    after = []
    for b, st in enumerate(states):
        fed = [int(x) & 0xFFFFFFFF if ids_a.dtype != np.int64 else int(x) for x in ids_a[b]]
        if lens is not None:
            fed = fed[:max(0, min(int(lens[b]), len(fed)))]
        want, row = ref.call(toks, tab, st, fed, n_words, end_ids, max_depth)
        assert [int(x) for x in r["state"][b]] == ref.state_row(want), (b, st, fed, [hex(int(x)) for x in r["state"][b]], want)
        assert r["mask"][b].tolist() == row.tolist(), (b, st, fed)
        assert int(r["live"][b]) == int(want[1]), (b, st, fed)
        after.append(want)
    return r, after


def dep_lists(dep_off, dep_ids):
    return [[int(t) for t in dep_ids[int(dep_off[q]):int(dep_off[q + 1])]] for q in range(len(dep_off) - 1)]


def check_index(index, name, sizes=(1, 2, 63, 64, 65), extra_words=(0,)):
    """The index of random tables -- ops of every kind, bytes that are no op, trans and ret values at and above their bounds, n_ret 0 -- and
    of the hand-made ones is the definition's bit for bit: rows (the zero words between n_words and stride included), some, dep_off and
    every dep entry."""
    v, specials, toks = vocab(name)
    al = dfa_cases.alphabet_of(toks) if name != "deps" else list(b"abc()[]\x00\xff")
    tabs = [("random%d" % n, random_table(n, al, 3, density=0.6 if n < 100 else 0.9)) for n in sizes]
    tabs += [("no ret", random_table(5, al, 4, n_ret=0)), ("paren", paren_table()), ("brackets", brackets_table())]
    seen = {"free": 0, "touch": 0}
    for label, tab in tabs:
        S = ref.n_states(tab)
        for extra in extra_words:
            nw = min_words(v) + extra
            want_rows, want_some, want_dep = ref.index(toks, tab, nw)
            rows, some, dep_off, dep_ids = index(ref.table_bytes(tab), S, ref.n_ret(tab), nw)
            assert rows.shape == want_rows.shape == (S, ref.stride(nw)), (label, rows.shape)
            assert (rows == want_rows).all(), (label, nw, np.argwhere(rows != want_rows)[:4].tolist())
            assert some.tolist() == want_some.tolist(), (label, nw)
            assert dep_lists(dep_off, dep_ids) == want_dep, (label, nw)
            assert (rows[:, nw:] == 0).all()
            seen["free"] += int(want_some.sum())
            seen["touch"] += sum(map(len, want_dep))
    assert seen["free"] and seen["touch"]
    return seen


DEP_LENGTHS = (0, 1, 63, 64, 65, 200)


def deps_table():
    """Over vocab_deps (a token per byte): state q < 6 pushes on the bytes below DEP_LENGTHS[q] and walks on every other byte, so its dep
    list has exactly that length; state 6 pops on every byte (256 entries); state 7 walks on the upper half only.  Pushes go to state 7
    or die (a target that is no state), pops return through two ret rows."""
    trans = np.full((8, 256), D, dtype=np.uint16)
    op = np.zeros((8, 256), dtype=np.uint8)
    for q, n in enumerate(DEP_LENGTHS):
        for x in range(256):
            if x < n:
                op[q, x] = ref.PUSH | (x % 16)
                trans[q, x] = 7 if x % 3 else 9
            else:
                trans[q, x] = (q + x) % 8 if x % 5 else D
    for x in range(256):
        op[6, x], trans[6, x] = ref.POP, x % 3                           # (ret row 2 does not exist)
        if x >= 128:
            trans[7, x] = x % 6
    ret = np.array([[(y * 3) % 8 if y % 4 else D for y in range(16)], [(y + 1) % 11 for y in range(16)]], dtype=np.uint16)
    return trans, ret, op, np.array([1, 0, 1, 0, 0, 1, 1, 0], dtype=np.uint8)


def check_deps(index, run):
    """NAMED CHECK (the mutant "dep": a dependent id tested against an empty stack must fail here).  dep lists of length 0, 1, 63, 64, 65,
    200 and 256, entry for entry, over ids on both sides of a row's piece boundary; dep_cap exact, larger, and one too small -- refused;
    then the masks of every state under an empty stack, a stack at max_depth (every push dies) and stacks whose top picks the pop's way."""
    v, specials, toks = vocab("deps")
    tab = deps_table()
    S, R, nw = 8, 2, min_words(v) + 1
    want_rows, want_some, want_dep = ref.index(toks, tab, nw)
    assert [len(d) for d in want_dep] == list(DEP_LENGTHS) + [256, 0]
    n_dep = sum(map(len, want_dep))
    for cap in (None, n_dep, n_dep + 3):
        rows, some, dep_off, dep_ids = index(ref.table_bytes(tab), S, R, nw, dep_cap=cap)
        assert (rows == want_rows).all() and some.tolist() == want_some.tolist() and dep_lists(dep_off, dep_ids[:n_dep]) == want_dep, cap
    try:
        index(ref.table_bytes(tab), S, R, nw, dep_cap=n_dep - 1)
        raise AssertionError("a dep_cap one too small was not refused")
    except TooSmall as e:
        assert e.args[0] == n_dep
    sp = 70150
    stacks = [(), (1,), (2, 5), (4,) * 3, (7, 8, 1, 2), (3, 8)]
    states = [ref.begin(q, st) for q in range(S) for st in stacks]
    lived = died = 0
    for max_depth in (4, 64):
        r, after = expect(run, toks, tab, rows_of(states), states, NO_IDS(len(states)), nw, (sp,), max_depth=max_depth)
        for s0, s1 in zip(states, after):
            ok = ref.allowed(toks, tab, s0, (sp,), max_depth)
            lived += len(ok & set(want_dep[s0[0]]))
            died += len(set(want_dep[s0[0]]) - ok)
        assert after[6 * len(stacks) + 5] == ref.BROKEN and after[6 * len(stacks) + 3][1]      # state 6: nothing but dependent ids; under (3, 8) none lives
    assert lived and died
    # a step along the masks: an id whose bit was set never breaks a sequence
    r, after = expect(run, toks, tab, rows_of(states), states, NO_IDS(len(states)), nw, (sp,))
    ids = []
    for s0 in after:
        ok = sorted(ref.allowed(toks, tab, s0, (sp,))) if s0[1] else [0]
        ids.append([ok[min(len(s0[4]), len(ok) - 1)]])
    for s0, t in zip(after, ids):
        assert not s0[1] or not ref.step(toks, tab, s0, t, (sp,))[2]
    expect(run, toks, tab, r["state"], after, ids, nw, (sp,), in_place=True)
    return n_dep


DEPTHS = (0, 1, 2, 15, 16, 17, 63, 64)


def check_stack(run):
    """NAMED CHECK (the mutant "pop": a pop that ignores the symbol and takes ret[v][0] must fail here).  Every probe id from every state
    of the bracket table under stacks of depth 0, 1, 2, 15, 16, 17, 63 and 64 -- the nibble-word boundaries -- whose tops are either kind of
    bracket, with max_depth 64 and with max_depth equal to the depth; max_depth 1; a token that pops three levels with two on the stack,
    one that pushes and pops inside itself; garbage nibbles above the depth, a depth above max_depth on load; state_out on state_in."""
    v, specials, toks = vocab("brackets")
    nw = min_words(v)
    tab = brackets_table()
    pool = heal_cases.probe_ids(v, specials)
    end = (25, 40)
    rng = random.Random(2)
    popped3 = inside = 0
    for depth in DEPTHS:
        for top in ((1, 1), (2, 2), (2, 1), (1, 2)):
            body = tuple(rng.choice((1, 2)) for _ in range(depth))
            stack = (body[:-2] + top)[-depth:] if depth >= 2 else (top[-depth:] if depth else ())
            assert len(stack) == depth
            for max_depth in sorted({64, max(depth, 1)}):
                pairs = [(ref.begin(q, stack), t) for q in (0, 1) for t in pool]
                states = [s for s, _ in pairs]
                r, after = expect(run, toks, tab, rows_of(states), states, [[t] for _, t in pairs], nw, end, max_depth=max_depth,
                                  in_place=(depth % 2 == 1))
                for (s, t), a in zip(pairs, after):
                    if v.get(t) == b")))" and depth == 2:
                        assert a == ref.BROKEN
                        popped3 += 1
                    if v.get(t) in (b"()", b"(a)") and a[1]:
                        assert a[4] == stack
                        inside += 1
            if not depth:
                break
    assert popped3 and inside
    # max_depth 1: one bracket may be open; a second opener is not in the mask
    s1 = [ref.begin(0), ref.begin(1, (1,)), ref.begin(0, (2,))]
    r, after = expect(run, toks, tab, rows_of(s1), s1, NO_IDS(3), nw, end, max_depth=1)
    assert bit(r["mask"][0], 1) and not bit(r["mask"][1], 1) and not bit(r["mask"][1], 3) and bit(r["mask"][1], 2) and not bit(r["mask"][2], 2) and bit(r["mask"][2], 4)
    assert not bit(r["mask"][1], 6) and bit(r["mask"][0], 6)                  # "()" pushes inside itself: not at the limit
    # rows no call writes: garbage nibbles above the depth are dropped, a depth above max_depth breaks the row
    raw = [ref.raw_row(0, con=True, depth=2, nibbles=(1, 2, 9, 9, 15) + (7,) * 59), ref.raw_row(0, con=True, depth=0, nibbles=(3,) * 64),
           ref.raw_row(1, con=True, depth=16, nibbles=(1,) * 16 + (5,) * 48), ref.raw_row(0, con=True, depth=17, nibbles=(2,) * 17 + (6,)),
           ref.raw_row(0, con=True, depth=65, nibbles=(1,) * 64), ref.raw_row(0, con=True, depth=127, nibbles=(1,) * 64),
           ref.raw_row(0, con=True, depth=9, nibbles=(1,) * 9), ref.raw_row(0, done=True, depth=5, nibbles=(1,) * 5),
           ref.raw_row(0, depth=5, nibbles=(1,) * 5), ref.raw_row(2, con=True, depth=1, nibbles=(1,))]
    states = [ref.row_state(x) for x in raw]
    for max_depth in (64, 8):
        r, after = expect(run, toks, tab, np.array(raw, dtype=np.uint64), states, NO_IDS(len(raw)), nw, end, max_depth=max_depth)
        assert after[0] == (0, True, False, False, (1, 2)) and after[1] == (0, True, False, False, ()) and after[4] == after[5] == ref.BROKEN
        assert after[7] == (0, False, False, True, ()) and after[8] == ref.FREE and after[9] == ref.BROKEN
        assert (after[6] == ref.BROKEN) == (max_depth == 8) and (after[2] == ref.BROKEN) == (max_depth == 8)
        assert [int(x) for x in r["state"][0]] == [0 | ref.CON | 2 << 24, 0x21, 0, 0, 0]
        expect(run, toks, tab, np.array(raw, dtype=np.uint64), states, [[2]] * len(raw), nw, end, max_depth=max_depth, in_place=True)


def check_end_depth(run):
    """NAMED CHECK (the mutant "end": END allowed at non-zero depth must fail here).  The paren table over the vocabulary "paren": END
    follows only an accepting state WITH AN EMPTY STACK -- in the mask and as a drawn id; END as an id of no token, as an ordinary id that
    also walks on (the ordinary rule wins) and in the last word of the row."""
    v, specials, toks = vocab("paren")
    nw = min_words(v)
    tab = paren_table()
    last = 32 * nw - 1
    end = (9, 1, last)                                                 # 9: no token; 1: ")" -- ordinary, and it walks on where a pop is possible
    states = [ref.begin(0), ref.begin(1, (0,)), ref.begin(1, (0, 1)), ref.begin(1), ref.begin(2), ref.begin(2, (1,)), ref.begin(1, (1,) * 64)]
    r, after = expect(run, toks, tab, rows_of(states), states, NO_IDS(len(states)), nw, end)
    assert [bit(r["mask"][b], 9) and bit(r["mask"][b], last) for b in range(len(states))] == [False, False, False, True, True, True, False]
    assert [bit(r["mask"][b], 1) for b in range(len(states))] == [False, True, True, True, True, True, True]      # (row 5 broke: ones)
    for t in (9, last, 1):
        _, a = expect(run, toks, tab, rows_of(states), states, [[t]] * len(states), nw, end)
        if t != 1:
            assert [(s[1], s[2], s[3]) for s in a] == [(False, True, False)] * 3 + [(False, False, True)] * 2 + [(False, True, False)] * 2, t
        else:                                                          # ")" walks where it can; where it cannot it is an END id: state 2 with an empty stack is done
            assert a[1] == (2, True, False, False, ()) and a[2] == (1, True, False, False, (0,)) and a[3] == (1, False, False, True, ()) and a[4][3]
    return True




def check_flags_and_layouts(run, index):
    """KEEP_FREE against a poisoned mask; int64 ids outside 32 bits; rows of 4k - 1, 4k and 4k + 1 words; state_out on state_in -- over a
    table with dependent ids (the ops-zero anchor runs tests/dfa_cases.py's own checks of the same)."""
    v, specials, toks = vocab("brackets")
    tab = brackets_table()
    base = min_words(v)
    k4 = (base + 4) // 4 * 4
    end = (25,)
    states = [ref.begin(0), ref.begin(1, (1,)), ref.FREE, ref.begin(0, (2, 1)), (0, False, False, True, ()), ref.begin(1, (2,))]
    for nw in sorted({base, k4 - 1, k4, k4 + 1, k4 + 4}):
        want = ref.index(toks, tab, nw)
        got = index(ref.table_bytes(tab), 2, 2, nw)
        assert (got[0] == want[0]).all() and got[1].tolist() == want[1].tolist() and dep_lists(got[2], got[3]) == want[2]
        r, after = expect(run, toks, tab, rows_of(states), states, NO_IDS(len(states)), nw, end + (32 * nw - 1,))
        ids = np.array([[2], [2], [2], [4], [2], [1 << 32 | 2]], dtype=np.int64)            # ")" | ")" | free | "]" against a ( on top | done | no id
        r2, after2 = expect(run, toks, tab, r["state"], after, ids, nw, end + (32 * nw - 1,), in_place=True)
        assert after2[0] == ref.BROKEN and after2[1] == (0, True, False, False, ()) and after2[3] == ref.BROKEN and after2[5] == ref.BROKEN
    nw = base
    init = np.arange(len(states) * nw, dtype=np.uint32).reshape(len(states), nw) + 77
    ids = [[2], [2], [2], [2], [2], [4]]
    r = run(ref.table_bytes(tab), 2, 2, ids=np.array(ids, dtype=np.int32), state=rows_of(states), flags=ref.KEEP_FREE, end_ids=end, n_words=nw, mask_init=init,
            max_depth=64)
    want = [ref.call(toks, tab, st, x, nw, end) for st, x in zip(states, ids)]
    assert r["live"].tolist() == [0, 1, 0, 1, 0, 0]
    for b, (st, row) in enumerate(want):
        assert [int(x) for x in r["state"][b]] == ref.state_row(st)
        assert r["mask"][b].tolist() == (row.tolist() if st[1] else init[b].tolist()), b
