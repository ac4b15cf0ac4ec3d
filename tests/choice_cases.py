"""Tables, states and CHECKS shared by tests/test_choice_cpu.py (the host simulation) and tests/test_gpu_choice.py (the kernel): every check
takes `run(table, ids=, state=, lengths=, flags=, end_ids=, n_words=, in_place=, mask_init=) -> dict(state, mask, live)` -- one call of
the code under test over one of tests/heal_cases.py's toy vocabularies -- and compares it with the definition of tests/choice_ref.py,
state rows bit for bit."""
import itertools
import random

import numpy as np

import choice_ref as ref
import heal_cases

TOYS = dict(heal_cases.TOYS, long=heal_cases.vocab_long)
NO_IDS = lambda n: np.zeros((n, 0), dtype=np.int32)


def toy(name):
    vocab, specials = TOYS[name]()
    return vocab, specials, ref.ordinary(vocab)


def min_words(vocab):
    return (max(vocab) + 32) // 32


def bit(row, t):
    return t < 32 * len(row) and bool((int(row[t >> 5]) >> (t & 31)) & 1)


def rows(states):
    return np.stack([ref.state_row(s) for s in states]) if len(states) else np.zeros((0, ref.STATE_WORDS), dtype=np.uint64)


def expect(run, toks, choices, raw_rows, states, ids, n_words, end_ids=(), then_free=False, **kw):
    """One call over `states` (as the rows raw_rows) and ids [B, K] (a list of lists, or an array with lengths in kw): state rows, masks and
    live bytes are the definition's.  Returns (the call's result, the states it left)."""
    ids_a = ids if isinstance(ids, np.ndarray) else np.array(ids, dtype=np.uint32).reshape(len(states), -1).view(np.int32)
    lens = kw.get("lengths")
    r = run(ref.table(choices), ids=ids_a, state=raw_rows, flags=ref.THEN_FREE if then_free else 0, end_ids=end_ids, n_words=n_words, **kw)
    after = []
    for b, st in enumerate(states):
        fed = [int(x) & 0xFFFFFFFF if ids_a.dtype != np.int64 else int(x) for x in ids_a[b]]
        if lens is not None:
            fed = fed[:max(0, min(int(lens[b]), len(fed)))]
        want, row = ref.call(toks, choices, st, fed, n_words, end_ids, then_free)
        assert r["state"][b].tolist() == ref.state_row(want).tolist(), (b, st, fed, ref.row_state(r["state"][b]), want)
        assert r["mask"][b].tolist() == row.tolist(), (b, st, fed)
        assert int(r["live"][b]) == int(bool(want[0])), (b, st, fed)
        after.append(want)
    return r, after


# ---------------------------------------------------------------------------------------------- tables
def strings_abc(top=4):
    return [bytes(t) for n in range(1, top + 1) for t in itertools.product(b"abc", repeat=n)]


def packed(strings):
    """Strings as tables of up to 64 slots with one selected slot per sequence: each sequence sees a one-slot table."""
    for i in range(0, len(strings), ref.SLOTS):
        part = strings[i:i + ref.SLOTS]
        yield part, [ref.begin(part, [s]) for s in range(len(part))]


def spellable(toks, rng, top=12):
    """A string some ids spell: a few ordinary tokens joined, cut to at most `top` bytes (so its last token may not fit)."""
    s = b""
    while len(s) < top and (not s or rng.random() < 0.7):
        s += rng.choice(toks)[1]
    return s[:rng.randrange(1, top + 1)] or s[:1]


def random_table(name, n, seed):
    vocab, specials, toks = toy(name)
    rng = random.Random(seed * 1000 + n)
    short = [t for t in toks if len(t[1]) <= 6]
    out = []
    for s in range(n):
        c = spellable(short, rng)
        if s and rng.random() < 0.3:                                  # shares a beginning with an earlier choice
            p = out[rng.randrange(len(out))]
            c = (p[:rng.randrange(1, len(p) + 1)] + c)[:20]
        out.append(c)
    return out


def tables(name):
    """(label, choices) of every table shape the checks walk: 2, 5, 63 and 64 random slots, empty slots in the middle, duplicates."""
    out = [("random%d" % n, random_table(name, n, 3)) for n in (2, 5, 63, 64)]
    holes = random_table(name, 9, 4)
    holes[2] = holes[3] = holes[6] = b""
    out.append(("holes", holes))
    dup = random_table(name, 6, 5)
    dup[4] = dup[1]
    dup[5] = dup[1] + dup[0][:1]
    out.append(("duplicates", dup))
    return out


def selections(choices, rng, n):
    """n selections over a table: all slots, single slots, random subsets, an empty one (a free row)."""
    full = [s for s, c in enumerate(choices) if c]
    out = [None, [], full[:1], full[-1:]]
    while len(out) < n:
        out.append(sorted(rng.sample(range(len(choices)), rng.randrange(1, len(choices) + 1))))
    return out[:n]


def reachable(toks, choices, end_ids, then_free, cap=40):
    """Constrained states reachable from the full selection and a few others by ids the masks allow (breadth first, at most cap)."""
    seen, queue = [], [ref.load(choices, ref.begin(choices)), ref.load(choices, ref.begin(choices, [0])), ref.load(choices, ref.begin(choices, range(0, len(choices), 2)))]
    while queue and len(seen) < cap:
        st = queue.pop(0)
        if not st[0] or st in seen:
            continue
        seen.append(st)
        for t in sorted(ref.allowed(toks, choices, st, end_ids, then_free)):
            queue.append(ref.step(toks, choices, st, [t], end_ids, then_free))
    return seen


def special_ids(name):
    """(a special id, an ordinary id, the id of the last bit of the last word) to serve as END ids"""
    vocab, specials, _ = toy(name)
    sp = min(specials) if specials else max(vocab) + 1
    return sp, min(vocab), 32 * min_words(vocab) - 1


# ---------------------------------------------------------------------------------------------- checks
def check_one_slot_strings(run, name, then_free=False, extra_words=0):
    """Every string of 1 .. 4 bytes over {a, b, c} as a one-slot table: the first masks.  NAMED CHECK: the mutants must fail here."""
    vocab, specials, toks = toy(name)
    nw = min_words(vocab) + extra_words
    end = (special_ids(name)[0],)
    for part, states in packed(strings_abc()):
        _, after = expect(run, toks, part, rows(states), states, NO_IDS(len(states)), nw, end, then_free)
    return after


def check_tables_and_walks(run, name, then_free, steps=10, B=48, seed=9):
    """The named tables: first masks of many selections, then random walks -- most ids obey the mask, some leave it -- one id a call, rows
    and masks compared at every step; an id is accepted iff its bit was set in the mask in front of it.  Then the same ids as [B, K] calls:
    whole, at every cut, with lengths."""
    vocab, specials, toks = toy(name)
    nw = min_words(vocab)
    sp, od, last = special_ids(name)
    pool = heal_cases.probe_ids(vocab, specials) + [last]
    accepted = refused = finished = 0
    for label, choices in tables(name):
        rng = random.Random(seed)
        end = (sp, last) if label != "random5" else (od, sp)
        sel = selections(choices, rng, B)
        start = [ref.begin(choices, s) for s in sel]
        r, states = expect(run, toks, choices, rows(start), start, NO_IDS(B), nw, end, then_free)
        fed = []
        for k in range(steps):
            ids = []
            for st in states:
                ok = sorted(ref.allowed(toks, choices, st, end, then_free)) if st[0] else []
                ids.append(rng.choice(ok) if ok and rng.random() < 0.88 else rng.choice(pool))
            prev_mask, prev = r["mask"], states
            r, states = expect(run, toks, choices, r["state"], prev, [[t] for t in ids], nw, end, then_free, in_place=(k % 2 == 0))
            for b, t in enumerate(ids):
                if prev[b][0]:                                        # constrained in front of the id
                    broke = ref.step(toks, choices, prev[b], [t], end, then_free)[2]
                    assert bit(prev_mask[b], t) == (not broke), (label, b, t, prev[b])
                    accepted += not broke
                    refused += broke
                else:
                    assert states[b] == prev[b]                       # free, done and broken rows read no ids
            fed.append(ids)
        finished += sum(s[3] for s in states)
        K = len(fed)
        by_seq = [[fed[k][b] for k in range(K)] for b in range(B)]
        whole, final = expect(run, toks, choices, rows(start), start, by_seq, nw, end, then_free)
        assert final == states
        for cut in (1, K // 2, K - 1):
            a, mid = expect(run, toks, choices, rows(start), start, [s[:cut] for s in by_seq], nw, end, then_free)
            b2, fin = expect(run, toks, choices, a["state"], mid, [s[cut:] for s in by_seq], nw, end, then_free, in_place=True)
            assert (b2["state"] == whole["state"]).all() and (b2["mask"] == whole["mask"]).all()
        lens = np.array([i % (K + 2) - 1 for i in range(B)], dtype=np.int32)      # -1 .. K: clamped to 0 .. K
        ids64 = np.array(by_seq, dtype=np.int64)
        expect(run, toks, choices, rows(start), start, ids64, nw, end, then_free, lengths=lens)
    assert accepted and refused and finished
    return accepted, refused, finished


def check_every_probe_id_from_every_state(run, name, then_free):
    vocab, specials, toks = toy(name)
    nw = min_words(vocab)
    sp, od, last = special_ids(name)
    pool = heal_cases.probe_ids(vocab, specials) + [last]
    for label, choices in tables(name)[:2] + tables(name)[4:]:
        end = (sp, od, last)
        states = reachable(toks, choices, end, then_free)
        assert len(states) >= 2
        pairs = [(st, t) for st in states for t in pool]
        expect(run, toks, choices, rows([st for st, _ in pairs]), [st for st, _ in pairs], [[t] for _, t in pairs], nw, end, then_free)


def check_long_and_edge_choices(run_for):
    """63 and 64 bytes; a choice whose every prefix is a token; choices at the edges of the byte order; a first byte no token spells.
    run_for(name): the run of a toy vocabulary."""
    run = run_for("long")
    vocab, specials, toks = toy("long")
    nw = min_words(vocab)
    choices = [b"a" * 63, b"a" * 64, b"a" * 63 + b"b", b"a" * 62 + b"b", b"b"]
    start = [ref.begin(choices, s) for s in (None, [0], [1], [2], [3], [1, 2], [4])]
    r, states = expect(run, toks, choices, rows(start), start, NO_IDS(len(start)), nw, (70,))
    assert ref.allowed(toks, choices, start[2], (70,)) == set(range(64))          # a .. a^64: 64 ids from one slot
    ids = [[62, 0], [62, 70], [63, 70], [62, 66], [61, 67], [64, 0], [67, 70]]       # a^63 a | a^63 END | a^64 END | a^63 a^63b | a^62 b | a^65 | b END
    r, states = expect(run, toks, choices, r["state"], states, ids, nw, (70,))
    assert [(s[3], s[4], s[2]) for s in states] == [(False, 0, False), (True, 0, False), (True, 1, False), (False, 0, True), (False, 0, False),
                                                   (False, 0, True), (True, 4, False)]
    run = run_for("chain")
    vocab, specials, toks = toy("chain")
    choices = [b"a" * 64, b"ab" * 32]
    start = [ref.begin(choices, s) for s in ([0], [1], None)]
    r, _ = expect(run, toks, choices, rows(start), start, NO_IDS(3), min_words(vocab), (80,))
    assert sum(bin(int(x)).count("1") for x in r["mask"][0]) == 64
    run = run_for("edges")
    vocab, specials, toks = toy("edges")
    choices = [b"\x00\x00\x00", b"\xff\xff\xff\xff", b"\x00\x01", b"\xff\x00", b"\xfe\xff", b"c\xff\xff", b"\x00"]
    start = [ref.begin(choices, [s]) for s in range(len(choices))] + [ref.begin(choices)]
    r, states = expect(run, toks, choices, rows(start), start, NO_IDS(len(start)), min_words(vocab), (31,))
    expect(run, toks, choices, r["state"], states, [[0], [1], [0], [2], [9], [6], [0], [2]], min_words(vocab), (31,))
    run = run_for("gaps")
    vocab, specials, toks = toy("gaps")
    choices = [b"bd", b"zz", b"ab", b"c"]                             # no token spells b, z or c alone
    start = [ref.begin(choices, s) for s in ([0], [1], [0, 1], [0, 2], [3], None)]
    r, states = expect(run, toks, choices, rows(start), start, NO_IDS(len(start)), min_words(vocab), (4,))
    assert [s[2] for s in states] == [True, True, True, False, True, False]
    assert (r["mask"][0] == 0xFFFFFFFF).all() and r["live"].tolist() == [0, 0, 0, 1, 0, 1]


def check_end_ids_and_flags(run, name="gaps"):
    vocab, specials, toks = toy(name)
    nw = min_words(vocab)
    sp, od, last = special_ids(name)
    choices = [b"a", b"ab", b"abc", b"aabc"]
    start = [ref.begin(choices)] * 8
    # END as a special, as the ordinary id 0 = "a" (which also spells "aabc"'s next byte: the ordinary reading wins), in the last word
    end = (sp, 0, last)
    ids = [[0, sp], [0, 0], [0, last], [0, 0, sp], [2, sp], [3, 0], [0, 5], [sp, 0]]
    ids = [x + [0x7FFFFFFF] * (3 - len(x)) for x in ids]
    lens = np.array([2, 2, 2, 3, 2, 2, 2, 2], dtype=np.int32)
    r, states = expect(run, toks, choices, rows(start), start, np.array(ids, dtype=np.int32), nw, end, lengths=lens)
    assert [(s[3], s[4], s[2], s[1]) for s in states] == [(True, 0, False, 1), (False, 0, False, 2), (True, 0, False, 1), (False, 0, True, 0),
                                                          (True, 1, False, 2), (True, 2, False, 3), (False, 0, True, 0), (False, 0, True, 0)]
    first = ref.mask(toks, choices, ref.step(toks, choices, start[0], [0], end), nw, end)
    assert all(bit(first, t) for t in end) and not bit(ref.mask(toks, choices, start[0], nw, end), sp)
    # THEN_FREE: done as soon as a slot is spelled out, the lowest such slot; END ids are not in the row
    r, states = expect(run, toks, choices, rows(start[:3]), start[:3], [[0, 0], [2, 0], [3, 0]], nw, end, then_free=True)
    assert [(s[3], s[4], s[1]) for s in states] == [(True, 0, 1), (True, 1, 2), (True, 2, 3)]
    dup = [b"ab", b"ab", b"abc"]
    _, states = expect(run, toks, dup, rows([ref.begin(dup)] * 2), [ref.begin(dup)] * 2, [[2], [3]], nw, (), then_free=True)
    assert [(s[3], s[4]) for s in states] == [(True, 0), (True, 2)]
    # KEEP_FREE against a poisoned mask: rows that are not constrained after the call keep what they held
    choices = [b"aab", b"c", b"zz"]
    start = [ref.begin(choices, s) for s in ([], [0], [0], [1], [2], [0])]
    init = np.arange(len(start) * nw, dtype=np.uint32).reshape(len(start), nw) + 77
    ids = [[0], [12], [sp], [0], [0], [0]]                            # free | "aab": nothing left but END | breaks | "a" is not "c" | nor "zz" | "a" of "aab"
    r = run(ref.table(choices), ids=np.array(ids, dtype=np.int32), state=rows(start), flags=ref.KEEP_FREE, end_ids=(sp,), n_words=nw, mask_init=init)
    want = [ref.call(toks, choices, st, x, nw, (sp,)) for st, x in zip(start, ids)]
    assert r["live"].tolist() == [0, 1, 0, 0, 0, 1]
    for b, (st, row) in enumerate(want):
        assert r["state"][b].tolist() == ref.state_row(st).tolist()
        assert r["mask"][b].tolist() == (row.tolist() if st[0] else init[b].tolist()), b


def check_layout(run, name="gaps"):
    """n_words at the minimum, + 1, a multiple of four and not; int32 and int64 ids; values that are no ids."""
    vocab, specials, toks = toy(name)
    choices = random_table(name, 7, 8)
    sp = special_ids(name)[0]
    start = [ref.begin(choices, s) for s in (None, [0], [1, 2], [], [3], [4, 5, 6])]
    base = min_words(vocab)
    for nw in sorted({base, base + 1, (base + 3) // 4 * 4, (base + 3) // 4 * 4 + 4, (base + 3) // 4 * 4 + 2}):
        last = 32 * nw - 1
        r, states = expect(run, toks, choices, rows(start), start, NO_IDS(len(start)), nw, (sp, last))
        ids = [sorted(ref.allowed(toks, choices, st, (sp, last)))[0] if st[0] else 0 for st in states]
        for dtype in (np.int32, np.int64):
            expect(run, toks, choices, r["state"], states, np.array(ids, dtype=dtype).reshape(-1, 1), nw, (sp, last), in_place=(dtype == np.int64))
    bad = [-1, -100, 1 << 32, (1 << 32) + int(min(vocab)), -(1 << 63)]
    st = [ref.begin(choices)] * len(bad)
    _, after = expect(run, toks, choices, rows(st), st, np.array([[x] for x in bad], dtype=np.int64), base, (sp,))
    assert all(s == ref.BROKEN for s in after)


def check_load_sanitation(run, name="gaps"):
    """Rows no call writes: A naming empty slots, slots shorter than k or with a length above 64, k = 127, done and broken rows."""
    vocab, specials, toks = toy(name)
    nw = min_words(vocab)
    choices = [b"ab", b"", b"abca", b"", b"a" * 64]
    raw = [ref.raw_row([0, 1, 3]), ref.raw_row([1, 3]), ref.raw_row([0, 2], 3), ref.raw_row([0], 3), ref.raw_row([4], 127), ref.raw_row([0, 2, 4], 127),
           ref.raw_row([0, 2], 2, done=True, hit=2), ref.raw_row([0, 2], 1, broken=True), ref.raw_row([], 100, done=True, hit=63), ref.raw_row([], 0),
           ref.raw_row(range(64)), ref.raw_row([0], 2, broken=True, done=True, hit=5)]
    states = [ref.row_state(x) for x in raw]
    r, after = expect(run, toks, choices, np.stack(raw), states, NO_IDS(len(raw)), nw, (4,))
    assert after[0] == (frozenset([0]), 0, False, False, 0) and after[1] == ref.FREE and after[2] == (frozenset([2]), 3, False, False, 0)
    assert after[3] == ref.FREE and after[4] == (frozenset([4]), 64, False, False, 0) and after[5] == after[4]
    assert after[6] == (frozenset(), 2, False, True, 2) and after[7] == ref.BROKEN and after[8] == (frozenset(), 64, False, True, 63)
    assert after[10][0] == frozenset([0, 2, 4]) and after[11] == ref.BROKEN
    assert r["state"][6].tolist() == [0, 2 | (1 << 9) | (2 << 16)] and r["state"][7].tolist() == [0, 1 << 8]
    # a length byte above 64 (no builder writes one): the slot is never a choice
    tab = ref.table(choices, lens=[2, 65, 4, 255, 64])
    r = run(tab, ids=NO_IDS(2), state=np.stack([ref.raw_row([1, 3]), ref.raw_row([0, 1, 3])]), flags=0, end_ids=(4,), n_words=nw)
    assert r["state"].tolist() == [[0, 0], [1, 0]] and r["live"].tolist() == [0, 1]
