"""Automata, states and CHECKS shared by tests/test_dfa_cpu.py (the host simulation) and tests/test_gpu_dfa.py (the kernels): every check
takes `run(table, n_states, ids=, state=, lengths=, flags=, end_ids=, n_words=, in_place=, mask_init=) -> dict(state, mask, live)` -- one
step call of the code under test over one of the toy vocabularies -- and / or `index(table, n_states, n_words) -> (rows, some)`, and
compares them with the definition of tests/dfa_ref.py, state words and index words bit for bit.  `table` is the table's bytes as they lie
in memory."""
import random
import re

import numpy as np

import choice_cases
import choice_ref
import dfa_ref as ref
import heal_cases

TOYS = choice_cases.TOYS
NO_IDS = choice_cases.NO_IDS
toy = choice_cases.toy
min_words = choice_cases.min_words
bit = choice_cases.bit
special_ids = choice_cases.special_ids


def compiled(pattern):
    """(trans, accept) of a pattern, by the product's compiler (tests/test_dfa_compile_cpu.py holds it against re.fullmatch)"""
    from splintr_amd import dfa
    d = dfa.compile_regex(pattern)
    return d.trans, d.accept


def alternation(strings):
    """(trans, accept) of "exactly one of these byte strings" """
    return compiled(b"|".join(re.escape(c) for c in strings if c))


def words(states):
    return np.array([ref.state_row(s) for s in states], dtype=np.uint64)


def expect(run, toks, tab, raw_words, states, ids, n_words, end_ids, **kw):
    """One call over `states` (as the words raw_words) and ids [B, K] (a list of lists, or an array with lengths in kw): state words, masks
    and live bytes are the definition's.  Returns (the call's result, the states it left)."""
    ids_a = ids if isinstance(ids, np.ndarray) else np.array(ids, dtype=np.uint32).reshape(len(states), -1).view(np.int32)
    lens = kw.get("lengths")
    r = run(ref.table_bytes(*tab), ref.n_states(tab), ids=ids_a, state=raw_words, end_ids=end_ids, n_words=n_words, **kw)
    after = []
    for b, st in enumerate(states):
        fed = [int(x) & 0xFFFFFFFF if ids_a.dtype != np.int64 else int(x) for x in ids_a[b]]
        if lens is not None:
            fed = fed[:max(0, min(int(lens[b]), len(fed)))]
        want, row = ref.call(toks, tab, st, fed, n_words, end_ids)
        assert int(r["state"][b]) == ref.state_row(want), (b, st, fed, ref.row_state(r["state"][b]), want)
        assert r["mask"][b].tolist() == row.tolist(), (b, st, fed)
        assert int(r["live"][b]) == int(want[1]), (b, st, fed)
        after.append(want)
    return r, after


# ---------------------------------------------------------------------------------------------- automata
JUNK = (0xFFFF, 0xFFFE, 0x8000)


def random_automaton(n, alphabet, seed, density=0.5):
    """n states over the bytes of `alphabet`: a transition is a random state, DEAD, or a value AT OR ABOVE n that must read as DEAD (n
    itself, n + 1, and values far above); every other byte holds such a value too.  Not trimmed: the index is defined for any table."""
    rng = random.Random(seed * 7919 + n)
    no_state = [n, n + 1] + [j for j in JUNK if j >= n]
    trans = np.random.RandomState(seed * 31 + n).choice(np.array(no_state, dtype=np.uint16), size=(n, 256))
    for q in range(n):
        for x in alphabet:
            trans[q, x] = rng.randrange(n) if rng.random() < density else rng.choice(no_state)
    accept = np.array([rng.random() < 0.3 for _ in range(n)], dtype=np.uint8)
    return trans, accept


def alphabet_of(toks):
    return sorted({x for _, b in toks for x in b})


def hand_automata(name):
    """(label, table) of the shapes the issue names, over the toy vocabulary `name`."""
    out = []
    D = ref.DEAD
    if name == "long":                                                # a*: a 128-byte token walked whole, from the one state
        t = np.full((1, 256), D, dtype=np.uint16)
        t[0, ord("a")] = 0
        out.append(("a*", (t, np.array([1], dtype=np.uint8))))
        t = np.full((130, 256), D, dtype=np.uint16)                  # a{0,129}: the 128-byte token fits from states 0 and 1 only
        for q in range(129):
            t[q, ord("a")] = q + 1
        out.append(("a{0,129}", (t, np.ones(130, dtype=np.uint8))))
    if name == "edges":                                               # transitions on 00 and on ff ff
        t = np.full((4, 256), D, dtype=np.uint16)
        t[0, 0x00], t[1, 0x00], t[0, 0xFF], t[2, 0xFF], t[3, 0x00], t[3, 0xFE] = 1, 1, 2, 3, 0, 3
        out.append(("00|ffff", (t, np.array([0, 1, 0, 1], dtype=np.uint8))))
    # state 1: an empty row that does not accept; state 2: accepts with no way on; state 3: an empty row that is no state's target
    t = np.full((4, 256), D, dtype=np.uint16)
    t[0, ord("a")], t[0, ord("b")], t[0, ord("c")] = 0, 2, 1
    t[1, ord("z")] = 0
    out.append(("dead ends", (t, np.array([0, 0, 1, 0], dtype=np.uint8))))
    return out


# ---------------------------------------------------------------------------------------------- checks
def check_index(index, name, sizes=(1, 2, 63, 64, 65), extra_words=(0,)):
    """NAMED CHECK (the mutant "first": a walk that tests only the first byte for DEAD must fail here): the index is bit for bit the
    definition's -- the some bytes and the zero words between n_words and stride included -- for random automata of the given sizes, with
    transitions at or above n_states that must read as DEAD, and the hand-made shapes."""
    vocab, specials, toks = toy(name)
    al = alphabet_of(toks)
    tabs = [("random%d" % n, random_automaton(n, al, 3, 0.6 if n < 100 else 0.9)) for n in sizes] + hand_automata(name)
    seen_bits = seen_dead_late = 0
    for label, tab in tabs:
        S = ref.n_states(tab)
        for extra in extra_words:
            nw = min_words(vocab) + extra
            want_rows, want_some = ref.index(toks, tab, nw)
            rows, some = index(ref.table_bytes(*tab), S, nw)
            assert rows.shape == want_rows.shape == (S, ref.stride(nw)), (label, rows.shape)
            assert (rows == want_rows).all(), (label, nw, np.argwhere(rows != want_rows)[:4].tolist())
            assert some.tolist() == want_some.tolist(), (label, nw)
            assert (rows[:, nw:] == 0).all()
            seen_bits += int(want_some.sum())
        # tokens whose first byte walks and a later one dies: what the mutant gets wrong
        seen_dead_late += sum(1 for q in range(min(S, 64)) for _, b in toks if len(b) > 1 and ref.walk(tab, q, b[:1]) != ref.DEAD and ref.walk(tab, q, b) == ref.DEAD)
    assert seen_bits and seen_dead_late
    return seen_bits, seen_dead_late


def check_against_choice(run, name, steps=8, B=24, seed=9):
    """The random choice tables of tests/choice_cases.py with all slots selected: the DFA of the alternation of the choices gives the same
    mask, live, done and broken as the guided-choice definition at every step of every walk, along and off the masks -- the new rule
    against one that is already pinned."""
    vocab, specials, toks = toy(name)
    nw = min_words(vocab)
    sp, od, last = special_ids(name)
    pool = heal_cases.probe_ids(vocab, specials) + [last]
    accepted = refused = finished = 0
    for label, choices in choice_cases.tables(name):
        rng = random.Random(seed)
        end = (sp, last) if label != "random5" else (od, sp)
        tab = alternation(choices)
        c_states = [choice_ref.load(choices, choice_ref.begin(choices))] * B
        d_states = [ref.begin(0)] * B
        r, d_states = expect(run, toks, tab, words(d_states), d_states, NO_IDS(B), nw, end)
        for k in range(steps + 1):
            for b in range(B):                                        # the two definitions side by side
                cs = choice_ref.settle(toks, choices, c_states[b], end)
                c_states[b] = cs
                assert r["mask"][b].tolist() == choice_ref.mask(toks, choices, cs, nw, end).tolist(), (label, k, b, cs)
                assert (int(r["live"][b]), d_states[b][3], d_states[b][2]) == (int(bool(cs[0])), cs[3], cs[2]), (label, k, b, cs, d_states[b])
            if k == steps:
                break
            ids = []
            for cs in c_states:
                ok = sorted(choice_ref.allowed(toks, choices, cs, end)) if cs[0] else []
                ids.append(rng.choice(ok) if ok and rng.random() < 0.85 else rng.choice(pool))
            prev_mask, prev = r["mask"], d_states
            r, d_states = expect(run, toks, tab, r["state"], prev, [[t] for t in ids], nw, end, in_place=(k % 2 == 0))
            c_states = [choice_ref.step(toks, choices, cs, [t], end) for cs, t in zip(c_states, ids)]
            for b, t in enumerate(ids):
                if prev[b][1]:                                        # constrained in front of the id: accepted iff its bit was set
                    broke = ref.step(toks, tab, prev[b], [t], end)[2]  # (the step alone: a state that then has nothing to draw breaks later)
                    assert bit(prev_mask[b], t) == (not broke), (label, b, t, prev[b])
                    accepted += not broke
                    refused += broke
        finished += sum(s[3] for s in d_states)
    assert accepted and refused and finished
    return accepted, refused, finished


PROBE_PATTERNS = {"chain": rb"(a|b){0,3}(ab)*a{4,6}", "gaps": rb"(ab|c)*a{1,3}(bc?)?", "edges": b"(\\\x00|\\\xff\\\xff|a|bc)*c\\\xff?", "long": rb"(aaaa)*(ab?|b)"}


def check_every_probe_id_from_every_state(run, name):
    """Every probe id -- the vocabulary, a special, ids of neither map, all-ones -- and int64 values outside 32 bits, from every state of an
    automaton (a trimmed minimal automaton: every state is reachable)."""
    vocab, specials, toks = toy(name)
    nw = min_words(vocab)
    sp, od, last = special_ids(name)
    pool = heal_cases.probe_ids(vocab, specials) + [last]
    tab = compiled(PROBE_PATTERNS[name])
    S = ref.n_states(tab)
    assert S >= 4
    end = (sp, od, last)
    pairs = [(ref.begin(q), t) for q in range(S) for t in pool]
    expect(run, toks, tab, words([s for s, _ in pairs]), [s for s, _ in pairs], [[t] for _, t in pairs], nw, end)
    wide = [1 << 32, (1 << 32) + int(min(vocab)), -1, -(1 << 63), (1 << 40) + sp]
    st = [ref.begin(q) for q in range(S) for _ in wide]
    _, after = expect(run, toks, tab, words(st), st, np.array([[x] for _ in range(S) for x in wide], dtype=np.int64), nw, end)
    assert all(s == ref.BROKEN for s in after)


def check_end_ids(run, name="gaps"):
    """NAMED CHECK (the mutant "end": END allowed without accept[q] must fail here).  a|ab|abc|aabc: END as a special, as the ordinary id 0
    = "a" (which also walks on towards "aabc": the ordinary rule wins), in the last word of the row; END too early."""
    vocab, specials, toks = toy(name)
    nw = min_words(vocab)
    sp, od, last = special_ids(name)
    tab = alternation([b"a", b"ab", b"abc", b"aabc"])
    start = [ref.begin(0)] * 9
    end = (sp, 0, last)
    ids = [[0, sp], [0, 0], [0, last], [0, 0, sp], [2, sp], [3, 0], [0, 5], [sp, 0], [0, 0, 0]]
    ids = [x + [0x7FFFFFFF] * (3 - len(x)) for x in ids]
    lens = np.array([2, 2, 2, 3, 2, 2, 2, 2, 3], dtype=np.int32)
    r, states = expect(run, toks, tab, words(start), start, np.array(ids, dtype=np.int32), nw, end, lengths=lens)
    #           a END     a a (on)   a END(last)  a a END (aa does not accept)  ab END   abc END("a": dead -> END)   a ca   END too early   a a a
    assert [(s[1], s[2], s[3]) for s in states] == [(False, False, True), (True, False, False), (False, False, True), (False, True, False),
                                                    (False, False, True), (False, False, True), (False, True, False), (False, True, False),
                                                    (False, True, False)]
    first = ref.mask(toks, tab, ref.step(toks, tab, start[0], [0], end), nw, end)
    assert all(bit(first, t) for t in end) and not bit(ref.mask(toks, tab, start[0], nw, end), sp) and not bit(ref.mask(toks, tab, start[0], nw, end), last)
    # every state of the automaton, no ids: the END bits are in the row iff the state accepts
    S = ref.n_states(tab)
    st = [ref.begin(q) for q in range(S)]
    r, _ = expect(run, toks, tab, words(st), st, NO_IDS(S), nw, (sp, last))
    held = [q for q in range(S) if r["live"][q]]                      # (a state with nothing to draw broke: its row is ones)
    assert [bit(r["mask"][q], sp) and bit(r["mask"][q], last) for q in held] == [bool(tab[1][q]) for q in held]
    assert any(tab[1][q] for q in held) and not all(tab[1][q] for q in held)
    # and END from every state
    expect(run, toks, tab, words(st), st, [[sp]] * S, nw, (sp, last))
    expect(run, toks, tab, words(st), st, [[last]] * S, nw, (sp, last))


def check_flags(run, name="gaps"):
    """KEEP_FREE against a poisoned mask; int32 and int64 ids; the state written in place."""
    vocab, specials, toks = toy(name)
    nw = min_words(vocab)
    sp = special_ids(name)[0]
    tab = alternation([b"aab", b"c", b"zz"])                          # no token spells c or z alone
    q_aa = ref.walk(tab, 0, b"aa")
    start = [ref.FREE, ref.begin(0), ref.begin(0), ref.begin(q_aa), ref.begin(0), (0, False, False, True)]
    init = np.arange(len(start) * nw, dtype=np.uint32).reshape(len(start), nw) + 77
    ids = [[0], [12], [sp], [0], [0], [0]]                            # free | "aab": only END is left | breaks | "a" behind "aa": breaks | "a" of "aab" | done: not read
    r = run(ref.table_bytes(*tab), ref.n_states(tab), ids=np.array(ids, dtype=np.int32), state=words(start), flags=ref.KEEP_FREE, end_ids=(sp,), n_words=nw,
            mask_init=init)
    want = [ref.call(toks, tab, st, x, nw, (sp,)) for st, x in zip(start, ids)]
    assert r["live"].tolist() == [0, 1, 0, 0, 1, 0]
    for b, (st, row) in enumerate(want):
        assert int(r["state"][b]) == ref.state_row(st)
        assert r["mask"][b].tolist() == (row.tolist() if st[1] else init[b].tolist()), b
    for dtype in (np.int32, np.int64):
        for in_place in (False, True):
            expect(run, toks, tab, words(start), start, np.array(ids, dtype=dtype), nw, (sp,), in_place=in_place)


def check_layout_and_load(run, index, name="gaps"):
    """n_words of 4k - 1, 4k and 4k + 1 (and the minimum); words no call writes: q that is no state, done and broken set together, bits
    that are not named."""
    vocab, specials, toks = toy(name)
    tab = compiled(PROBE_PATTERNS[name])
    S = ref.n_states(tab)
    sp = special_ids(name)[0]
    base = min_words(vocab)
    k4 = (base + 4) // 4 * 4
    for nw in sorted({base, k4 - 1, k4, k4 + 1, k4 + 4}):
        last = 32 * nw - 1
        rows, some = index(ref.table_bytes(*tab), S, nw)
        want_rows, want_some = ref.index(toks, tab, nw)
        assert (rows == want_rows).all() and some.tolist() == want_some.tolist()
        st = [ref.begin(q) for q in range(S)] + [ref.FREE]
        r, states = expect(run, toks, tab, words(st), st, NO_IDS(len(st)), nw, (sp, last))
        ids = [sorted(ref.allowed(toks, tab, s, (sp, last)))[-1] if s[1] else 0 for s in states]
        expect(run, toks, tab, r["state"], states, np.array(ids, dtype=np.int64).reshape(-1, 1), nw, (sp, last), in_place=True)
    raw = [ref.raw_row(S, con=True), ref.raw_row(0xFFFF, con=True), ref.raw_row(S - 1, con=True), ref.raw_row(1, con=True, done=True),
           ref.raw_row(1, con=True, broken=True, done=True), ref.raw_row(2, broken=True), ref.raw_row(3), ref.raw_row(S + 7, done=True),
           ref.raw_row(1, con=True, extra=1 << 40), ref.raw_row(0, extra=0xFF << 56)]
    states = [ref.row_state(x) for x in raw]
    r, after = expect(run, toks, tab, np.array(raw, dtype=np.uint64), states, NO_IDS(len(raw)), base, (sp,))
    assert after[0] == ref.BROKEN and after[1] == ref.BROKEN and after[3] == (1, False, False, True) and after[4] == ref.BROKEN
    assert after[5] == ref.BROKEN and after[6] == ref.FREE and after[7] == (S + 7, False, False, True) and after[9] == ref.FREE
    assert int(r["state"][3]) == 1 | ref.DONE and int(r["state"][4]) == ref.BRK and int(r["state"][8]) == ref.state_row(after[8]) and int(r["state"][9]) == 0
    # ids behind a done, a broken and a free word are not read
    expect(run, toks, tab, np.array(raw, dtype=np.uint64), states, [[0]] * len(raw), base, (sp,))
