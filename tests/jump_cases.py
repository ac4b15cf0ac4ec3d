"""Automata, jump tables and CHECKS shared by tests/test_dfa_jump_cpu.py (the host simulation) and tests/test_gpu_dfa_jump.py (the
kernels).  Every check takes some of

    runs(table, n_states) -> (run uint8 [S, 64], run_len uint8 [S])                      the force and runs launches
    run(table, n_states, ids=, state=, jump_index=, row_len_out=, lengths=, flags=, end_ids=, n_words=, in_place=, mask_init=)
        -> dict(state, mask, live, forced int32 [B, row_len_out], forced_len int32 [B])   one jump call; forced arrives filled with
                                                                                          FORCED_POISON, which every entry at and beyond
                                                                                          forced_len must still hold
    step(table, n_states, ids=, state=, lengths=, flags=, end_ids=, n_words=, ...) -> dict(state, mask, live)    the plain step

of the code under test over one of the toy vocabularies, and compares them with the definition of tests/jump_ref.py, bit for bit.
`table` is the table's bytes as they lie in memory, `jump_index` a jump index's (tests/jump_ref.py: pack_index)."""
import random
import re

import numpy as np

import dfa_cases
import dfa_ref as ref
import heal_cases
import jump_ref as jref

TOYS = dfa_cases.TOYS
NO_IDS = dfa_cases.NO_IDS
toy = dfa_cases.toy
min_words = dfa_cases.min_words
special_ids = dfa_cases.special_ids
words = dfa_cases.words
compiled = dfa_cases.compiled
FORCED_POISON = -0x5A5A5A5B
D = ref.DEAD


def expect(run, toks, tab, raw_words, states, ids, jidx, row_len_out, n_words, end_ids, **kw):
    """One jump call over `states` (as the words raw_words), ids [B, K] and the jump index jidx: state words, masks, live bytes, the
    emitted ids and their counts are the definition's; what lies behind a count was not written.  Returns (the result, the states left,
    the emitted ids)."""
    S = ref.n_states(tab)
    ids_a = ids if isinstance(ids, np.ndarray) else np.array(ids, dtype=np.uint32).reshape(len(states), -1).view(np.int32)
    lens = kw.get("lengths")
    j_ids, j_n, _, _ = jref.index_parts(jidx, S)
    r = run(ref.table_bytes(*tab), S, ids=ids_a, state=raw_words, jump_index=jidx, row_len_out=row_len_out, end_ids=end_ids, n_words=n_words, **kw)
    after, out = [], []
    for b, st in enumerate(states):
        fed = [int(x) & 0xFFFFFFFF if ids_a.dtype != np.int64 else int(x) for x in ids_a[b]]
        if lens is not None:
            fed = fed[:max(0, min(int(lens[b]), len(fed)))]
        want, row, emitted = jref.call(toks, tab, st, fed, j_ids, j_n, row_len_out, n_words, end_ids)
        assert int(r["state"][b]) == ref.state_row(want), (b, st, fed, ref.row_state(r["state"][b]), want)
        assert r["mask"][b].tolist() == row.tolist(), (b, st, fed)
        assert int(r["live"][b]) == int(want[1]), (b, st, fed)
        m = int(r["forced_len"][b])
        assert m == len(emitted), (b, st, fed, m, emitted)
        assert [int(x) & 0xFFFFFFFF for x in r["forced"][b][:m]] == emitted, (b, st, fed)
        assert (r["forced"][b][m:] == FORCED_POISON).all(), (b, "an entry at or beyond forced_len was written")
        after.append(want)
        out.append(emitted)
    return r, after, out


# ---------------------------------------------------------------------------------------------- automata
def forced_automaton(n, alphabet, seed):
    """n states over the bytes of `alphabet`, most with ONE live byte (so runs are long, meet cycles and the cap), some with two or
    none, a third accepting; every other entry holds a value at or above n that must read as DEAD."""
    rng = random.Random(seed * 104729 + n)
    no_state = [n, n + 1] + [j for j in dfa_cases.JUNK if j >= n]
    trans = np.random.RandomState(seed * 17 + n).choice(np.array(no_state, dtype=np.uint16), size=(n, 256))
    for q in range(n):
        k = rng.choice([1, 1, 1, 1, 1, 2, 0, 3])
        for x in rng.sample(list(alphabet), min(k, len(alphabet))):
            trans[q, x] = rng.randrange(n)
    accept = np.array([rng.random() < 0.3 for _ in range(n)], dtype=np.uint8)
    return trans, accept


def cycle_automaton():
    """Two states forcing each other, none accepting: the run ends at the cap."""
    t = np.full((2, 256), D, dtype=np.uint16)
    t[0, ord("a")], t[1, ord("b")] = 1, 0
    return t, np.zeros(2, dtype=np.uint8)


def chain_automaton(data, accept_last=True, extra=()):
    """A chain spelling `data` from state 0; extra: (state, byte, to) transitions on top."""
    n = len(data) + 1
    t = np.full((n, 256), D, dtype=np.uint16)
    for i, x in enumerate(data):
        t[i, x] = i + 1
    for q, x, to in extra:
        t[q, x] = to
    acc = np.zeros(n, dtype=np.uint8)
    acc[n - 1] = 1 if accept_last else 0
    return t, acc


UTF8_CHAINS = [b"ab\xc3", b"ab\xc3\xa9", b"\xe2\x82", b"\xe2\x82\xac", b"\xf0\x9f\x8c", b"\xf0\x9f\x8c\x8d", b"\xa9x\xc3", b"\x80\x80\x80", b"\xc3\xa9\xe2",
               b"a\xe2\x82\xacb\xf0\x9f", b"\xff", b"\xf8\x80\x80", b"\xf8\x80\x80\x80", b"\xc3\x80\x80\x80\x80", b"\xe2x\x82"]


# ---------------------------------------------------------------------------------------------- checks
def check_runs(runs, name, sizes=(1, 2, 63, 64, 65)):
    """NAMED CHECK (the mutant "accept": a force that ignores accept[q] must fail here): run and run_len of every state are the
    definition's, zeros behind a run -- for automata with mostly forced states of the given sizes (transitions at or above n_states read
    as DEAD), a forced cycle, chains that end inside UTF-8 characters, and chains of 63 .. 70 bytes around the cap."""
    vocab, specials, toks = toy(name)
    al = dfa_cases.alphabet_of(toks)
    tabs = [("forced%d" % n, forced_automaton(n, al, 5)) for n in sizes] + [("cycle", cycle_automaton())]
    tabs += [("utf8 %r" % c, chain_automaton(c, extra=[(len(c), ord("p"), 0), (len(c), ord("q"), 0)])) for c in UTF8_CHAINS]
    tabs += [("a^%d" % n, chain_automaton(b"a" * n)) for n in (63, 64, 65, 70)]
    tabs += [("a^62 e2 82 ac", chain_automaton(b"a" * 62 + b"\xe2\x82\xac")), ("a^61 e2 82 ac", chain_automaton(b"a" * 61 + b"\xe2\x82\xac"))]
    seen_forced = seen_accepting_single = seen_capped = seen_trimmed = 0
    for label, tab in tabs:
        S = ref.n_states(tab)
        want, want_len = jref.run_arrays(tab)
        got, got_len = runs(ref.table_bytes(*tab), S)[:2]
        assert got_len.tolist() == want_len.tolist(), (label, np.argwhere(got_len != want_len)[:4].tolist())
        assert (got == want).all(), (label, np.argwhere(got != want)[:4].tolist())
        for q in range(min(S, 128)):
            live = int((tab[0][q] < S).sum())
            seen_forced += jref.force(tab, q) is not None
            seen_accepting_single += bool(tab[1][q]) and live == 1
            raw = jref.raw_run(tab, q)
            seen_capped += len(raw) == jref.MAX_BYTES
            seen_trimmed += len(jref.trim(raw)) < len(raw)
    assert seen_forced and seen_accepting_single and seen_capped and seen_trimmed
    return seen_forced, seen_accepting_single, seen_capped, seen_trimmed


JUMP_PATTERNS = {"chain": rb"ab(a|b)aab(ab)*bbb", "gaps": rb"abc(ab|c)cabbc[ab]bb", "edges": b"ab\\\x00\\\x00(a|b)c\\\xffcc", "long": rb"a{70}(b|ab)a{5}b"}


def reference_index(name, tab):
    return jref.index_of(toy(name)[2], tab)


def check_jump(run, name, row_lens=(1, 3, 16, 64)):
    """The jump step against the definition: a compiled pattern with forced stretches and the jump index the definition gives it (the
    runs, spelled greedily); from every state with no id, with every probe id, and along a walk of draws from the masks until every
    sequence is done -- at every width of the forced rows."""
    vocab, specials, toks = toy(name)
    nw = min_words(vocab)
    sp, od, last = special_ids(name)
    tab = compiled(JUMP_PATTERNS[name])
    S = ref.n_states(tab)
    jidx = reference_index(name, tab)
    j_n = jref.index_parts(jidx, S)[1]
    assert int((j_n > 0).sum()) >= 3 and (j_n == 0).any()
    end = (sp, last)
    pool = heal_cases.probe_ids(vocab, specials) + [last]
    emitted_total = 0
    for K in row_lens:
        st = [ref.begin(q) for q in range(S)] + [ref.FREE, ref.BROKEN, (1, False, False, True)]
        _, _, out = expect(run, toks, tab, words(st), st, NO_IDS(len(st)), jidx, K, nw, end)
        assert out[-1] == out[-2] == out[-3] == []                                  # free, broken, done: nothing is emitted
        emitted_total += sum(len(o) for o in out)
        pairs = [(ref.begin(q), t) for q in range(S) for t in pool]
        expect(run, toks, tab, words([s for s, _ in pairs]), [s for s, _ in pairs], [[t] for _, t in pairs], jidx, K, nw, end, in_place=True)
    # a walk: jump, draw from the mask, until done
    rng = random.Random(11)
    B = 24
    states = [ref.begin(0)] * B
    r, states, out = expect(run, toks, tab, words(states), states, NO_IDS(B), jidx, 3, nw, end)
    texts = [b"".join(dict(toks)[i] for i in o) for o in out]
    draws = 0
    for _ in range(40):
        if not any(s[1] for s in states):
            break
        ids = []
        for b, s in enumerate(states):
            ok = sorted(ref.allowed(toks, tab, s, end)) if s[1] else [0]
            t = rng.choice(ok)
            ids.append(t)
            if s[1] and t not in end:
                texts[b] += dict(toks)[t]
            draws += s[1]
        r, states, out = expect(run, toks, tab, r["state"], states, [[t] for t in ids], jidx, 3, nw, end, in_place=True)
        for b, o in enumerate(out):
            texts[b] += b"".join(dict(toks)[i] for i in o)
    # (a vocabulary that lacks single bytes has dead ends: such a sequence breaks; every other one is done, and what it spelled matches)
    assert all(s[3] or s[2] for s in states) and sum(s[3] for s in states) >= B // 4, states
    assert all(re.fullmatch(JUMP_PATTERNS[name], t) for s, t in zip(states, texts) if s[3]), texts[:3]
    assert emitted_total and draws
    return emitted_total, draws


def check_adversarial(run, name="gaps"):
    """NAMED CHECK (the mutant "nowalk": emission without the walk must fail here).  Jump tables no build would write: an id that does
    not walk in the middle of a row (the emission stops there, the sequence is not broken); a special and an id above the vocabulary; an
    id of all ones; n_ids of 200 over a row of ids that walk for ever; widths 1, 3 and 64; the sampler's ids as int64 with values outside
    32 bits in front of the jump."""
    vocab, specials, toks = toy(name)
    nw = min_words(vocab)
    sp, od, last = special_ids(name)
    by = {bytes(b): i for i, b in reversed(toks)}
    a, ab, bb = by[b"a"], by[b"ab"], by[b"bb"]
    # (ab)*bb...: state 0 loops on "ab" for ever
    t = np.full((3, 256), D, dtype=np.uint16)
    t[0, ord("a")], t[1, ord("b")], t[0, ord("b")], t[2, ord("b")] = 1, 0, 2, 0
    tab = (t, np.array([1, 0, 0], dtype=np.uint8))
    S = 3
    ids = np.zeros((S, 64), dtype=np.uint32)
    n_ids = np.zeros(S, dtype=np.int64)
    ids[0, :] = ab; n_ids[0] = 200                                                # 64 ids that walk, a count far above the row
    ids[1, :5] = [bb, ab, sp, ab, ab]; n_ids[1] = 5                                # state 1 wants "b": "bb" walks 1 -> 0 -> 2; "ab" from 2 does not walk
    ids[2, :4] = [max(vocab) + 1000, ab, ab, ab]; n_ids[2] = 4                     # an id above the vocabulary first: nothing is emitted
    jidx = jref.pack_index(ids, n_ids & 0xFF)
    end = (sp, last)
    st = [ref.begin(0), ref.begin(1), ref.begin(2)]
    for K in (1, 3, 64):
        _, after, out = expect(run, toks, tab, words(st), st, NO_IDS(3), jidx, K, nw, end)
        assert out[0] == [ab] * min(K, 64) and out[1] == [bb] and out[2] == []
        assert after[0] == ref.begin(0) and after[1] == ref.begin(2) and after[2] == ref.begin(2)      # stopping breaks nothing
    ids2 = ids.copy()
    ids2[1, :4] = [bb, sp, ab, ab]                                                 # a special (not ordinary) in the middle
    ids2[2, :3] = [0xFFFFFFFF, ab, ab]
    ids2[0, 2] = a                                                                 # "a" walks 0 -> 1; "ab" from 1 does not: stops after three
    jidx2 = jref.pack_index(ids2, [64, 4, 3])
    _, after, out = expect(run, toks, tab, words(st), st, NO_IDS(3), jidx2, 64, nw, end)
    assert out[0] == [ab, ab, a] and after[0] == ref.begin(1) and out[1] == [bb] and out[2] == []
    # the sampler's ids first, as int64: a value outside 32 bits breaks the sequence and nothing is emitted; "a" moves to state 1, whose row is used
    wide = np.array([[1 << 32], [a], [(1 << 40) + ab], [-1], [ab]], dtype=np.int64)
    st5 = [ref.begin(0)] * 5
    _, after, out = expect(run, toks, tab, words(st5), st5, wide, jidx, 16, nw, end)
    assert [s == ref.BROKEN for s in after] == [True, False, True, True, False]
    assert out[0] == out[2] == out[3] == [] and out[1] == [bb] and out[4] == [ab] * 16
    return True


def check_keep_free_and_layouts(run, name="gaps"):
    """KEEP_FREE against a poisoned mask; n_words of 4k - 1, 4k and 4k + 1; int32 and int64 ids; the state written in place."""
    vocab, specials, toks = toy(name)
    sp, od, last = special_ids(name)
    tab = compiled(JUMP_PATTERNS[name])
    S = ref.n_states(tab)
    jidx = reference_index(name, tab)
    j_ids, j_n, _, _ = jref.index_parts(jidx, S)
    base = min_words(vocab)
    k4 = (base + 4) // 4 * 4
    st = [ref.begin(q) for q in range(S)] + [ref.FREE, ref.BROKEN]
    for nw in sorted({base, k4 - 1, k4, k4 + 1, k4 + 4}):
        end = (sp, 32 * nw - 1)
        for dtype in (np.int32, np.int64):
            expect(run, toks, tab, words(st), st, np.zeros((len(st), 0), dtype=dtype), jidx, 16, nw, end, in_place=dtype == np.int64)
    nw = base
    init = np.arange(len(st) * nw, dtype=np.uint32).reshape(len(st), nw) + 77
    ids = [[od]] * len(st)                                                        # an ordinary id: some states walk, most break
    r = run(ref.table_bytes(*tab), S, ids=np.array(ids, dtype=np.int32), state=words(st), jump_index=jidx, row_len_out=16, flags=ref.KEEP_FREE, end_ids=(sp,),
            n_words=nw, mask_init=init)
    want = [jref.call(toks, tab, s, x, j_ids, j_n, 16, nw, (sp,)) for s, x in zip(st, ids)]
    assert any(w[0][1] for w in want) and not all(w[0][1] for w in want)
    for b, (s, row, emitted) in enumerate(want):
        assert int(r["state"][b]) == ref.state_row(s) and int(r["live"][b]) == int(s[1])
        assert r["mask"][b].tolist() == (row.tolist() if s[1] else init[b].tolist()), b
        assert [int(x) for x in r["forced"][b][:int(r["forced_len"][b])]] == emitted


def check_zero_index_is_the_step(run, step, name="gaps"):
    """With every n_ids zero the call is the plain step word for word: states, masks and live bytes of the two agree over every probe id
    from every state, with lengths, END ids and both id widths -- whatever the ids of the jump index hold."""
    vocab, specials, toks = toy(name)
    nw = min_words(vocab)
    sp, od, last = special_ids(name)
    tab = compiled(dfa_cases.PROBE_PATTERNS[name])
    S = ref.n_states(tab)
    pool = heal_cases.probe_ids(vocab, specials) + [last]
    pairs = [(ref.begin(q), t) for q in range(S) for t in pool] + [(ref.FREE, 0), (ref.BROKEN, 0), ((1, False, False, True), 0)]
    zero = jref.pack_index(np.full((S, 64), od, dtype=np.uint32), np.zeros(S, dtype=np.uint8))
    st = words([s for s, _ in pairs])
    for dtype in (np.int32, np.int64):
        ids = np.array([[t, od] for _, t in pairs], dtype=np.uint32).astype(dtype)
        lens = np.array([1 + (i % 2) for i in range(len(pairs))], dtype=np.int32)
        a = run(ref.table_bytes(*tab), S, ids=ids, state=st, jump_index=zero, row_len_out=16, lengths=lens, end_ids=(sp, od, last), n_words=nw)
        b = step(ref.table_bytes(*tab), S, ids=ids, state=st, lengths=lens, end_ids=(sp, od, last), n_words=nw)
        assert a["state"].tolist() == b["state"].tolist() and (a["mask"] == b["mask"]).all() and a["live"].tolist() == b["live"].tolist()
        assert (a["forced_len"] == 0).all() and (a["forced"] == FORCED_POISON).all()
