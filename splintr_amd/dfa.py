"""Regular expression -> deterministic automaton over BYTES, for the regex guide (include/splintr_hip.h, spl_dfa_step_device; DESIGN.md
4.18).  Pure Python, no dependency beyond numpy.

    compile_regex(pattern) -> ByteDFA        trans uint16 [S, 256] (DEAD = 0xFFFF), accept uint8 [S], start state 0
    stack([d0, d1, ...])   -> (ByteDFA, starts)   several automata in one table, the start state of each

The semantics are those of Python's `re` in BYTES mode with `fullmatch`: a str pattern is encoded to UTF-8 first, so a non-ASCII literal is
its bytes, `.` is any byte but \\n, and \\d \\w \\s are ASCII.  Supported: literals and escapes, `.`, classes with ranges and negation over
bytes, \\d \\w \\s \\D \\W \\S, groups `(...)` and `(?:...)`, alternation, `* + ? {m} {m,} {m,n}`.  Refused with a ValueError that names the
construct: anchors, look-around, back-references, lazy and possessive quantifiers, inline flags, a non-ASCII character inside a class, an
empty language, more than 4096 states.

Construction: Thompson NFA -> subset construction over classes of bytes the pattern cannot tell apart -> TRIMMING (every state that cannot
reach an accepting state becomes DEAD, so a surviving state can always be completed: that is what makes "the walk does not die" the right
mask rule) -> Moore minimisation -> breadth-first numbering from the start state, which becomes 0.

UTF-8 validity of `.` and of negated classes is NOT this module's job: they admit any byte, so a guide alone may allow a token that ends
inside a character.  DeviceStreamingDecoder.allowed_mask(mask, and_into=True) ANDs the UTF-8 rows in afterwards, as for token healing and
guided choice."""
from typing import List, Sequence, Tuple, Union

import numpy as np

DEAD = 0xFFFF
MAX_STATES = 4096
_MAX_NFA = 1 << 18           # NFA states a pattern may expand to (counted repetitions are copied)
_MAX_SUBSETS = 1 << 16       # DFA states in front of the minimisation
_ALL = (1 << 256) - 1


def _set(*items) -> int:
    m = 0
    for it in items:
        if isinstance(it, tuple):
            for x in range(it[0], it[1] + 1):
                m |= 1 << x
        else:
            m |= 1 << it
    return m


_DIGIT = _set((0x30, 0x39))
_WORD = _set((0x30, 0x39), (0x41, 0x5A), (0x61, 0x7A), 0x5F)
_SPACE = _set(0x20, 0x09, 0x0A, 0x0D, 0x0C, 0x0B)
_CLASS_ESC = {ord("d"): _DIGIT, ord("D"): _ALL & ~_DIGIT, ord("w"): _WORD, ord("W"): _ALL & ~_WORD, ord("s"): _SPACE, ord("S"): _ALL & ~_SPACE}
_CHAR_ESC = {ord("n"): 0x0A, ord("t"): 0x09, ord("r"): 0x0D, ord("f"): 0x0C, ord("v"): 0x0B, ord("a"): 0x07}
_HEX = b"0123456789abcdefABCDEF"


class _Parser:
    """Pattern bytes -> a tree: ("set", mask) | ("cat", [nodes]) | ("alt", [nodes]) | ("rep", node, lo, hi or None)."""

    def __init__(self, pat: bytes, is_str: bool):
        self.p, self.i, self.is_str = pat, 0, is_str

    def fail(self, what: str, at=None):
        raise ValueError("unsupported in a regex guide: %s (at byte %d of the pattern)" % (what, self.i if at is None else at))

    def peek(self):
        return self.p[self.i] if self.i < len(self.p) else None

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):
            self.fail("an unbalanced ')'")
        return node

    def alt(self):
        branches = [self.cat()]
        while self.peek() == 0x7C:                                    # |
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self):
        items = []
        while self.peek() is not None and self.peek() not in (0x7C, 0x29):
            items.append(self.quantified())
        return ("cat", items)

    def quantified(self):
        at = self.i
        node = self.atom()
        c = self.peek()
        if c == 0x2A:
            lo, hi = 0, None
            self.i += 1
        elif c == 0x2B:
            lo, hi = 1, None
            self.i += 1
        elif c == 0x3F:
            lo, hi = 0, 1
            self.i += 1
        elif c == 0x7B:
            q = self.braces()
            if q is None:
                return node                                           # (a '{' that opens no quantifier is a literal, as in re)
            lo, hi = q
        else:
            return node
        nxt = self.peek()
        if nxt == 0x3F:
            self.fail("a lazy quantifier", at)
        if nxt == 0x2B:
            self.fail("a possessive quantifier", at)
        if nxt == 0x2A or (nxt == 0x7B and self._is_braces()):
            self.fail("a multiple repeat", at)
        if hi is not None and hi < lo:
            self.fail("a repetition {m,n} with n < m", at)
        return ("rep", node, lo, hi)

    def _is_braces(self):
        save = self.i
        q = self.braces()
        self.i = save
        return q is not None

    def braces(self):
        """'{m}', '{m,}', '{m,n}', '{,n}', '{,}' at the cursor -> (lo, hi) with the cursor behind the '}', or None with the cursor unmoved."""
        j = self.i + 1
        k = j
        while k < len(self.p) and 0x30 <= self.p[k] <= 0x39:
            k += 1
        lo_s = self.p[j:k]
        hi_s = None
        if k < len(self.p) and self.p[k] == 0x2C:
            m = k + 1
            while m < len(self.p) and 0x30 <= self.p[m] <= 0x39:
                m += 1
            hi_s = self.p[k + 1:m]
            k = m
        if k >= len(self.p) or self.p[k] != 0x7D or (not lo_s and hi_s is None):
            return None
        self.i = k + 1
        lo = int(lo_s) if lo_s else 0
        hi = lo if hi_s is None else (int(hi_s) if hi_s else None)
        return lo, hi

    def atom(self):
        c = self.peek()
        at = self.i
        if c == 0x28:                                                 # (
            self.i += 1
            if self.peek() == 0x3F:
                n = self.p[self.i + 1] if self.i + 1 < len(self.p) else None
                if n == 0x3A:
                    self.i += 2
                elif n in (0x3D, 0x21):
                    self.fail("a look-ahead (?= / (?!", at)
                elif n == 0x3C and self.i + 2 < len(self.p) and self.p[self.i + 2] in (0x3D, 0x21):
                    self.fail("a look-behind (?<= / (?<!", at)
                elif n == 0x50 and self.i + 2 < len(self.p) and self.p[self.i + 2] == 0x3D:
                    self.fail("a back-reference (?P=name)", at)
                elif n == 0x3E:
                    self.fail("an atomic group (?>", at)
                elif n in (0x50, 0x3C):
                    self.fail("a named group", at)
                elif n == 0x28:
                    self.fail("a conditional (?(", at)
                elif n == 0x23:
                    self.fail("a comment group (?#", at)
                else:
                    self.fail("inline flags (?...)", at)
            node = self.alt()
            if self.peek() != 0x29:
                self.fail("a group that is not closed", at)
            self.i += 1
            return node
        if c in (0x2A, 0x2B, 0x3F):
            self.fail("a quantifier with nothing to repeat")
        if c == 0x5E:
            self.fail("the anchor ^")
        if c == 0x24:
            self.fail("the anchor $")
        if c == 0x2E:
            self.i += 1
            return ("set", _ALL & ~(1 << 0x0A))
        if c == 0x5B:
            return ("set", self.klass())
        if c == 0x5C:
            kind, v = self.escape(False)
            return ("set", v if kind == "set" else 1 << v)
        self.i += 1
        return ("set", 1 << c)

    def escape(self, in_class: bool):
        """The escape at the cursor -> ("set", mask) or ("chr", byte); the cursor moves behind it."""
        at = self.i
        self.i += 1
        c = self.peek()
        if c is None:
            self.fail("a pattern that ends in a backslash", at)
        self.i += 1
        if c in _CLASS_ESC:
            return "set", _CLASS_ESC[c]
        if c == ord("x"):
            h = self.p[self.i:self.i + 2]
            if len(h) != 2 or h[0] not in _HEX or h[1] not in _HEX:
                self.fail("an incomplete \\x escape", at)
            self.i += 2
            return "chr", int(h, 16)
        if c == ord("0"):
            v, n = 0, 0
            while n < 2 and self.peek() is not None and 0x30 <= self.peek() <= 0x37:
                v, n = v * 8 + self.peek() - 0x30, n + 1
                self.i += 1
            return "chr", v
        if 0x31 <= c <= 0x39:
            self.fail("a back-reference \\%d" % (c - 0x30), at)
        if c == ord("b") and in_class:
            return "chr", 0x08
        if c in (ord("b"), ord("B")):
            self.fail("the word boundary \\%s" % chr(c), at)
        if c in (ord("A"), ord("Z")):
            self.fail("the anchor \\%s" % chr(c), at)
        if c in _CHAR_ESC:
            return "chr", _CHAR_ESC[c]
        if (0x41 <= c <= 0x5A) or (0x61 <= c <= 0x7A) or (0x30 <= c <= 0x39):
            self.fail("the escape \\%s" % chr(c), at)
        if c >= 0x80 and self.is_str and in_class:
            self.fail("a non-ASCII character inside a class", at)
        return "chr", c

    def klass(self) -> int:
        at = self.i
        self.i += 1
        neg = self.peek() == 0x5E
        if neg:
            self.i += 1
        m, first = 0, True
        while True:
            c = self.peek()
            if c is None:
                self.fail("a class that is not closed", at)
            if c == 0x5D and not first:
                self.i += 1
                break
            first = False
            lo = self._class_item()
            if isinstance(lo, tuple):                                 # \d and its kin: no range
                m |= lo[0]
                continue
            if self.peek() == 0x2D and self.i + 1 < len(self.p) and self.p[self.i + 1] != 0x5D:
                self.i += 1
                hi = self._class_item()
                if isinstance(hi, tuple):
                    self.fail("a class range that ends in a class escape", at)
                if hi < lo:
                    self.fail("a class range that runs backwards", at)
                m |= _set((lo, hi))
            else:
                m |= 1 << lo
        return (_ALL & ~m) if neg else m

    def _class_item(self):
        c = self.peek()
        if c == 0x5C:
            kind, v = self.escape(True)
            return (v,) if kind == "set" else v
        if c >= 0x80 and self.is_str:
            self.fail("a non-ASCII character inside a class")
        self.i += 1
        return c


class _Nfa:
    def __init__(self):
        self.eps: List[List[int]] = []
        self.edge: List[List[Tuple[int, int]]] = []               # (byte set, target)

    def new(self) -> int:
        if len(self.eps) >= _MAX_NFA:
            raise ValueError("unsupported in a regex guide: a pattern that expands to more than %d NFA states" % _MAX_NFA)
        self.eps.append([])
        self.edge.append([])
        return len(self.eps) - 1

    def build(self, node) -> Tuple[int, int]:
        """Thompson: a fragment with one entry and one exit."""
        kind = node[0]
        if kind == "set":
            a, b = self.new(), self.new()
            if node[1]:
                self.edge[a].append((node[1], b))
            return a, b
        if kind == "cat":
            a = b = self.new()
            for it in node[1]:
                x, y = self.build(it)
                self.eps[b].append(x)
                b = y
            return a, b
        if kind == "alt":
            a, b = self.new(), self.new()
            for it in node[1]:
                x, y = self.build(it)
                self.eps[a].append(x)
                self.eps[y].append(b)
            return a, b
        _, sub, lo, hi = node
        a = b = self.new()
        for _ in range(lo):
            x, y = self.build(sub)
            self.eps[b].append(x)
            b = y
        if hi is None:                                                # sub*
            x, y = self.build(sub)
            loop, out = self.new(), self.new()
            self.eps[b].append(loop)
            self.eps[loop] += [x, out]
            self.eps[y].append(loop)
            b = out
        else:
            out = self.new()
            for _ in range(hi - lo):                                  # (sub (sub (sub)?)?)?
                x, y = self.build(sub)
                self.eps[b] += [x, out]
                b = y
            self.eps[b].append(out)
            b = out
        return a, b


def _byte_classes(nfa: _Nfa) -> Tuple[List[int], List[int]]:
    """A representative byte of every class of bytes that no edge of the NFA tells apart, and the class of each byte."""
    sets = sorted({m for es in nfa.edge for m, _ in es})
    sig = {}
    cls = [0] * 256
    reps = []
    for x in range(256):
        s = tuple((m >> x) & 1 for m in sets)
        if s not in sig:
            sig[s] = len(reps)
            reps.append(x)
        cls[x] = sig[s]
    return reps, cls


def _subsets(nfa: _Nfa, start: int, final: int, reps):
    closure_of = {}

    def closure(states):
        out, stack = set(states), list(states)
        while stack:
            s = stack.pop()
            for t in nfa.eps[s]:
                if t not in out:
                    out.add(t)
                    stack.append(t)
        return frozenset(out)

    def closure1(s):
        if s not in closure_of:
            closure_of[s] = closure([s])
        return closure_of[s]

    s0 = closure1(start)
    ids = {s0: 0}
    order = [s0]
    trans = []
    i = 0
    while i < len(order):
        S = order[i]
        i += 1
        edges = [(m, t) for s in S for m, t in nfa.edge[s]]
        row = []
        for r in reps:
            T = set()
            for m, t in edges:
                if (m >> r) & 1:
                    T |= closure1(t)
            if not T:
                row.append(-1)
                continue
            T = frozenset(T)
            if T not in ids:
                if len(order) >= _MAX_SUBSETS:
                    raise ValueError("unsupported in a regex guide: more than %d states (the subset construction passed %d)" % (MAX_STATES, _MAX_SUBSETS))
                ids[T] = len(order)
                order.append(T)
            row.append(ids[T])
        trans.append(row)
    accept = [final in S for S in order]
    return trans, accept


def _trim(trans, accept):
    """States that cannot reach an accepting state become -1 (DEAD) everywhere."""
    n = len(trans)
    back = [[] for _ in range(n)]
    for s, row in enumerate(trans):
        for t in row:
            if t >= 0:
                back[t].append(s)
    good = [bool(a) for a in accept]
    stack = [s for s in range(n) if good[s]]
    while stack:
        t = stack.pop()
        for s in back[t]:
            if not good[s]:
                good[s] = True
                stack.append(s)
    return [[t if t >= 0 and good[t] else -1 for t in row] if good[s] else None for s, row in enumerate(trans)], good


def _minimise(trans, accept, good):
    """Moore: split blocks by (block, blocks of the successors) until nothing splits.  Returns block of every live state."""
    live = [s for s in range(len(trans)) if good[s]]
    block = {s: int(accept[s]) for s in live}
    n_blocks = len(set(block.values()))
    while True:
        sig = {}
        new = {}
        for s in live:
            k = (block[s], tuple(block[t] if t >= 0 else -1 for t in trans[s]))
            if k not in sig:
                sig[k] = len(sig)
            new[s] = sig[k]
        block = new
        if len(sig) == n_blocks:
            return block
        n_blocks = len(sig)


class ByteDFA:
    """A deterministic automaton over bytes: trans uint16 [S, 256] (DEAD = 0xFFFF: no way on), accept uint8 [S], start (0 from
    compile_regex).  Every state reaches an accepting state."""

    def __init__(self, trans: np.ndarray, accept: np.ndarray, start: int = 0, pattern=None):
        self.trans, self.accept, self.start, self.pattern = trans, accept, int(start), pattern

    @property
    def n_states(self) -> int:
        return int(self.trans.shape[0])

    def walk(self, q: int, data: bytes) -> int:
        """The state behind `data` from state q, DEAD as soon as a byte has no way on."""
        for x in data:
            if q == DEAD:
                break
            q = int(self.trans[q, x])
        return q

    def matches(self, data: bytes) -> bool:
        q = self.walk(self.start, data)
        return q != DEAD and bool(self.accept[q])

    def table(self) -> np.ndarray:
        """uint8 [S * 512 + S]: the table of spl_dfa_index_device / spl_dfa_step_device (little-endian uint16 trans[S][256], then accept[S])."""
        return np.concatenate([np.ascontiguousarray(self.trans, dtype="<u2").view(np.uint8).reshape(-1), np.ascontiguousarray(self.accept, dtype=np.uint8)])

    def longest(self, q: int = None):
        """The bytes of the longest match from state q (default: the start), None where matches are unbounded (a cycle is reachable)."""
        nxt = [sorted({int(t) for t in row if t != DEAD}) for row in self.trans]
        memo, on_path = {}, set()

        def depth(s):
            if s in memo:
                return memo[s]
            if s in on_path:
                raise OverflowError
            on_path.add(s)
            best = 0
            for t in nxt[s]:
                best = max(best, 1 + depth(t))
            on_path.discard(s)
            memo[s] = best
            return best

        import sys
        limit = sys.getrecursionlimit()
        sys.setrecursionlimit(max(limit, 4 * self.n_states + 1000))
        try:
            return depth(self.start if q is None else int(q))
        except OverflowError:
            return None
        finally:
            sys.setrecursionlimit(limit)

    def __repr__(self) -> str:
        return "ByteDFA(n_states=%d, start=%d%s)" % (self.n_states, self.start, "" if self.pattern is None else ", pattern=%r" % (self.pattern,))


def compile_regex(pattern: Union[str, bytes]) -> ByteDFA:
    """The minimal trimmed DFA over bytes of `pattern` under re.fullmatch in bytes mode (a str pattern: its UTF-8).  ValueError names what
    is not supported (see the module's docstring), an empty language and more than 4096 states."""
    if isinstance(pattern, str):
        pat, is_str = pattern.encode("utf-8"), True
    elif isinstance(pattern, (bytes, bytearray)):
        pat, is_str = bytes(pattern), False
    else:
        raise TypeError("pattern must be str or bytes, not %s" % type(pattern).__name__)
    tree = _Parser(pat, is_str).parse()
    nfa = _Nfa()
    start, final = nfa.build(tree)
    reps, cls = _byte_classes(nfa)
    trans, accept = _subsets(nfa, start, final, reps)
    trans, good = _trim(trans, accept)
    if not good[0]:
        raise ValueError("unsupported in a regex guide: an empty language (the pattern matches nothing)")
    block = _minimise(trans, accept, good)
    # one state per block, numbered breadth first from the start's block, bytes in order
    member = {}
    for s in sorted(block):
        member.setdefault(block[s], s)
    number = {block[0]: 0}
    queue = [block[0]]
    for b in queue:
        for t in trans[member[b]]:
            if t >= 0 and block[t] not in number:
                number[block[t]] = len(number)
                queue.append(block[t])
    n = len(number)
    if n > MAX_STATES:
        raise ValueError("unsupported in a regex guide: more than %d states (the minimal automaton has %d)" % (MAX_STATES, n))
    small = np.full((n, len(reps)), DEAD, dtype=np.uint16)
    acc = np.zeros(n, dtype=np.uint8)
    for b, k in number.items():
        s = member[b]
        acc[k] = 1 if accept[s] else 0
        for c, t in enumerate(trans[s]):
            if t >= 0:
                small[k, c] = number[block[t]]
    return ByteDFA(np.ascontiguousarray(small[:, np.array(cls)]), acc, 0, pattern)


def stack(dfas: Sequence[ByteDFA]) -> Tuple[ByteDFA, List[int]]:
    """Several automata laid into ONE table -> (the table as a ByteDFA whose start is the first automaton's, the start state of each).
    A sequence picks its automaton by the start state written into its state word.  ValueError above 4096 states in all."""
    dfas = list(dfas)
    if not dfas:
        raise ValueError("stack needs at least one automaton")
    total = sum(d.n_states for d in dfas)
    if total > MAX_STATES:
        raise ValueError("unsupported in a regex guide: more than %d states (the stacked automata have %d)" % (MAX_STATES, total))
    trans = np.full((total, 256), DEAD, dtype=np.uint16)
    accept = np.zeros(total, dtype=np.uint8)
    starts, base = [], 0
    for d in dfas:
        n = d.n_states
        t = d.trans.astype(np.uint32)
        trans[base:base + n] = np.where(t < n, t + base, DEAD).astype(np.uint16)
        accept[base:base + n] = d.accept
        starts.append(base + d.start)
        base += n
    return ByteDFA(trans, accept, starts[0], [d.pattern for d in dfas]), starts
