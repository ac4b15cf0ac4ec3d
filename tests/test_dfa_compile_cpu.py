"""splintr_amd/dfa.py against Python's `re` in bytes mode with fullmatch -- the semantics it claims: for every pattern every byte string of
length 0 .. 5 over a six-byte alphabet drawn from the pattern's own literals plus one foreign byte, 500 strings sampled by walking the
automaton to an accepting state, and 500 one-byte mutations of those; every state reaches an accepting state; minimal sizes that can be
derived by hand; every refusal with the construct named; stack."""
import itertools
import random
import re

import numpy as np
import pytest

from splintr_amd import dfa

PATTERNS = {
    "date": r"\d{4}-\d{2}-\d{2}",
    "float": r"-?(0|[1-9]\d*)(\.\d+)?([eE][+-]?\d+)?",
    "ipv4": r"((25[0-5]|2[0-4]\d|1\d\d|[1-9]?\d)\.){3}(25[0-5]|2[0-4]\d|1\d\d|[1-9]?\d)",
    "uuid": r"[0-9a-f]{8}-[0-9a-f]{4}-[0-9a-f]{4}-[0-9a-f]{4}-[0-9a-f]{12}",
    "email": r"[a-z0-9._%+-]+@[a-z0-9-]+(\.[a-z0-9-]+)*\.[a-z]{2,6}",
    "json": r'\{"name": "[^"\\]{1,16}", "score": -?(0|[1-9]\d{0,3})(\.\d{1,2})?, "tags": \[("[a-z]{1,8}"(, "[a-z]{1,8}"){0,3})?\]\}',
    "suffix": r"(a|b)*a(a|b){10}",
    "string": r'[^"\\]*',
    "counted": r"a{0,3}b?",
    "overlap": r"(?:ab|a)(?:c|bc)",
    "classes": r"\w+\s\d*",
    "escapes": r"\x41\.\t[\]\-a\\]{2}\S\D\W",
    "dot": r"a.c|.{0,2}",
    "utf8": "é+|[a-c]ü{2}",
    "empty branch": r"(|ab)c{,2}d{1,}",
    "brace literal": r"a{,}b{x{2}",
}
ALPHABETS = {                                                         # five bytes of the pattern's own literals and one foreign byte
    "date": b"0-91x\n", "float": b"0-.e1x", "ipv4": b"25.01x", "uuid": b"0-afg\xff", "email": b"a@.-0X", "json": b'{"a:1x', "suffix": b"abAB\x00z",
    "string": b'a"\\ \xff\n', "counted": b"abAB\x00c", "overlap": b"abcABx", "classes": b"a_ 1\t-", "escapes": b"A.\t]-\\", "dot": b"ac\nb\x00\xff",
    "utf8": b"\xc3\xa9\xbcacx", "empty branch": b"abcdxe", "brace literal": b"a{,}bx",
}
COMPILED = {}


def compiled(name):
    if name not in COMPILED:
        COMPILED[name] = dfa.compile_regex(PATTERNS[name])
    return COMPILED[name]


def rx(name):
    p = PATTERNS[name]
    return re.compile(p.encode("utf-8") if isinstance(p, str) else p)


def sample(d, rng, cap=200):
    """A string the automaton accepts: a random walk that stops at an accepting state (every state reaches one: trimmed)."""
    q, out = d.start, bytearray()
    while True:
        if d.accept[q] and (rng.random() < 0.25 or len(out) >= cap or not (d.trans[q] != dfa.DEAD).any()):
            return bytes(out)
        nxt = np.flatnonzero(d.trans[q] != dfa.DEAD)
        if len(out) >= cap:                                           # head for an accepting state: a byte that shortens the way
            nxt = [x for x in nxt if DIST[id(d)][int(d.trans[q, x])] < DIST[id(d)][q]] or nxt
        x = int(nxt[rng.randrange(len(nxt))])
        out.append(x)
        q = int(d.trans[q, x])


DIST = {}


def distances(d):
    """bytes to the nearest accepting state, per state (None: none reaches one)"""
    dist = [0 if a else None for a in d.accept]
    changed = True
    while changed:
        changed = False
        for q in range(d.n_states):
            best = min((dist[int(t)] + 1 for t in set(d.trans[q].tolist()) if t != dfa.DEAD and dist[int(t)] is not None), default=None)
            if best is not None and (dist[q] is None or best < dist[q]):
                dist[q], changed = best, True
    return dist


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_agrees_with_re_fullmatch(name):
    d, r = compiled(name), rx(name)
    al = ALPHABETS[name]
    assert len(set(al)) == 6, (name, al)
    n = 0
    for k in range(6):
        for t in itertools.product(al, repeat=k):
            s = bytes(t)
            assert d.matches(s) == (r.fullmatch(s) is not None), (name, s)
            n += 1
    assert n == sum(6 ** k for k in range(6))
    DIST[id(d)] = distances(d)
    rng = random.Random(sorted(PATTERNS).index(name) * 131 + 7)
    hits = misses = 0
    for _ in range(500):
        s = sample(d, rng)
        assert r.fullmatch(s) is not None, (name, s)
        hits += 1
        m = bytearray(s)
        kind = rng.randrange(3) if m else 1
        if kind == 0:
            m[rng.randrange(len(m))] = rng.randrange(256)
        elif kind == 1:
            m.insert(rng.randrange(len(m) + 1), rng.choice(al))
        else:
            del m[rng.randrange(len(m))]
        m = bytes(m)
        ok = r.fullmatch(m) is not None
        assert d.matches(m) == ok, (name, m)
        misses += not ok
    assert hits == 500 and misses


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_every_state_reaches_an_accepting_state_and_is_reached(name):
    d = compiled(name)
    assert d.start == 0 and d.trans.dtype == np.uint16 and d.trans.shape == (d.n_states, 256) and d.accept.shape == (d.n_states,)
    assert all(x is not None for x in distances(d))
    assert ((d.trans < d.n_states) | (d.trans == dfa.DEAD)).all()
    seen, queue = {0}, [0]
    for q in queue:
        for t in set(d.trans[q].tolist()):
            if t != dfa.DEAD and t not in seen:
                seen.add(t)
                queue.append(t)
    assert len(seen) == d.n_states
    # minimal: no two states agree on acceptance and on every byte's successor
    assert len({(int(d.accept[q]), d.trans[q].tobytes()) for q in range(d.n_states)}) == d.n_states
    tab = d.table()
    assert tab.dtype == np.uint8 and tab.size == d.n_states * 513 and tab[:2].tolist() == [int(d.trans[0, 0]) & 0xFF, int(d.trans[0, 0]) >> 8]


def test_minimal_sizes_derived_by_hand():
    # date: ten bytes in a row, no choice anywhere: a state in front of each byte and one behind the last
    assert compiled("date").n_states == 11
    # uuid: 36 bytes in a row
    assert compiled("uuid").n_states == 37
    # (a|b)*a(a|b){10}: the automaton must remember which of the last 11 bytes were "a": 2 ** 11 sets
    assert compiled("suffix").n_states == 2048
    assert compiled("string").n_states == 1 and compiled("date").longest() == 10 and compiled("uuid").longest() == 36
    assert compiled("suffix").longest() is None and compiled("counted").longest() == 4


@pytest.mark.parametrize("pattern, word", [
    (r"^a", "anchor ^"), (r"a$", "anchor $"), (r"\Aa", r"anchor \A"), (r"a\Z", r"anchor \Z"), (r"\bword", r"word boundary \b"), (r"a\Bb", r"word boundary \B"),
    (r"(?=a)a", "look-ahead"), (r"a(?!b)", "look-ahead"), (r"(?<=a)b", "look-behind"), (r"(?<!a)b", "look-behind"),
    (r"(a)\1", "back-reference"), (r"(?P<x>a)(?P=x)", "named group"), (r"(?P=x)", "back-reference"),
    (r"a*?", "lazy quantifier"), (r"a+?", "lazy quantifier"), (r"a??", "lazy quantifier"), (r"a{2,3}?", "lazy quantifier"),
    (r"a*+", "possessive quantifier"), (r"a++", "possessive quantifier"), (r"a{2}+", "possessive quantifier"),
    (r"(?i)a", "inline flags"), (r"(?s:a.)", "inline flags"), (r"(?>a)", "atomic group"),
    ("[é]", "non-ASCII character inside a class"), ("[a-é]", "non-ASCII character inside a class"), ("[^ü]", "non-ASCII character inside a class"),
    (r"[^\x00-\xff]", "empty language"), (r"a[^\x00-\xff]b|[^\d\D]", "empty language"),
    (r"(a|b)*a(a|b){12}", "more than 4096 states (the minimal automaton has 8192)"),
    (r"(a", "not closed"), (r"a)", "unbalanced"), (r"[a", "class that is not closed"), (r"*a", "nothing to repeat"), (r"a**", "multiple repeat"),
    (r"a{3,2}", "n < m"), (r"\q", r"escape \q"), ("a\\", "ends in a backslash"), (r"[z-a]", "runs backwards"), (r"\xg1", r"incomplete \x"),
])
def test_refusals_name_the_construct(pattern, word):
    with pytest.raises(ValueError) as e:
        dfa.compile_regex(pattern)
    assert word in str(e.value) and "unsupported in a regex guide" in str(e.value), str(e.value)


def test_bytes_patterns_and_types():
    d = dfa.compile_regex(b"[\xe9\xfc]+\\\xff")                       # a bytes pattern may put any byte into a class
    assert d.matches(b"\xe9\xfc\xff") and not d.matches(b"\xff") and d.n_states == 3
    assert dfa.compile_regex("é").matches("é".encode()) and dfa.compile_regex("é").n_states == 3
    with pytest.raises(TypeError):
        dfa.compile_regex(5)


def test_stack_start_states_and_disjoint_ranges():
    ds = [compiled("date"), compiled("counted"), compiled("uuid")]
    table, starts = dfa.stack(ds)
    assert starts == [0, 11, 16] and table.n_states == 11 + 5 + 37 and table.start == 0
    base = 0
    for d, s in zip(ds, starts):
        part = table.trans[base:base + d.n_states]
        live = part != dfa.DEAD
        assert ((part[live] >= base) & (part[live] < base + d.n_states)).all()           # no transition leaves the automaton's own range
        assert (live == (d.trans != dfa.DEAD)).all() and (part[live] - base == d.trans[live]).all()
        assert (table.accept[base:base + d.n_states] == d.accept).all()
        base += d.n_states
    for s, d, text in zip(starts, ds, (b"2026-10-21", b"aab", b"01234567-89ab-cdef-0123-456789abcdef")):
        q = table.walk(s, text)
        assert q != dfa.DEAD and table.accept[q]
        for other in starts:
            if other != s:
                assert table.walk(other, text) == dfa.DEAD or not table.accept[table.walk(other, text)]
    with pytest.raises(ValueError, match="more than 4096 states"):
        dfa.stack([compiled("suffix")] * 3)
    with pytest.raises(ValueError, match="at least one"):
        dfa.stack([])
