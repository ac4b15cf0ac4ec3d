"""Nest tables for spl_nest_index_device / spl_nest_step_device (include/splintr_hip.h): a byte automaton whose
transitions may PUSH a 4-bit symbol or POP one -- regular pieces inside nested brackets.  Pure Python and numpy.

    NestTable(trans, op, ret, accept, start=0)   trans uint16 [S, 256] (DEAD = 0xFFFF), op uint8 [S, 256] (0, PUSH | y, POP), ret uint16
                                                 [n_ret, 16], accept uint8 [S]
    from_dfa(ByteDFA) -> NestTable               every op zero: the regex guide's automaton
    json_table(top=, ws=) -> NestTable           RFC 8259 as json.loads reads it with NaN and Infinity refused, hand-built

One byte x from (q, stack), v = trans[q][x], o = op[q][x]: o == 0 goes to v; o == PUSH | y goes to v and pushes y (while the stack is
below max_depth); o == POP pops y and goes to ret[v][y]; anything that cannot be done is DEAD.  A word is accepted iff the walk ends in
an accepting state with an empty stack."""
from typing import Optional, Tuple

import numpy as np

DEAD = 0xFFFF
PUSH, POP = 0x10, 0x20
MAX_STATES, MAX_RET, MAX_DEPTH = 4096, 4096, 64


class NestTable:
    def __init__(self, trans, op, ret, accept, start: int = 0):
        trans, op, accept = np.asarray(trans), np.asarray(op), np.asarray(accept)
        ret = np.asarray(ret, dtype=np.uint16).reshape(-1, 16)
        if trans.dtype != np.uint16 or trans.ndim != 2 or trans.shape[1] != 256 or not 1 <= trans.shape[0] <= MAX_STATES:
            raise ValueError(f"trans must be a uint16 array of shape [n_states, 256] with n_states in 1 .. {MAX_STATES}")
        if op.dtype != np.uint8 or op.shape != trans.shape:
            raise ValueError("op must be a uint8 array of the shape of trans")
        if accept.shape != (trans.shape[0],):
            raise ValueError("accept must have one entry per state")
        if ret.shape[0] > MAX_RET:
            raise ValueError(f"ret must have at most {MAX_RET} rows of 16")
        if not 0 <= int(start) < trans.shape[0]:
            raise ValueError("start must be a state")
        self.trans, self.op, self.ret, self.accept, self.start = trans, op, ret, (accept != 0).astype(np.uint8), int(start)

    @property
    def n_states(self) -> int:
        return int(self.trans.shape[0])

    @property
    def n_ret(self) -> int:
        return int(self.ret.shape[0])

    def step(self, q: int, stack: Tuple[int, ...], byte: int, max_depth: int = MAX_DEPTH) -> Optional[Tuple[int, Tuple[int, ...]]]:
        """One byte from (q, stack) -> (q', stack'), None for DEAD.  stack: a tuple of symbols, the bottom first."""
        v, o = int(self.trans[q, byte]), int(self.op[q, byte])
        S = self.n_states
        if o == 0:
            return (v, stack) if v < S else None
        if o & 0xF0 == PUSH:
            return (v, stack + (o & 15,)) if v < S and len(stack) < max_depth else None
        if o == POP:
            if not stack or v >= self.n_ret:
                return None
            r = int(self.ret[v, stack[-1]])
            return (r, stack[:-1]) if r < S else None
        return None

    def walk(self, q: int, stack, data: bytes, max_depth: int = MAX_DEPTH):
        """(q, stack) behind `data`, None as soon as a byte is DEAD."""
        at = (int(q), tuple(stack))
        for x in data:
            at = self.step(at[0], at[1], x, max_depth)
            if at is None:
                return None
        return at

    def ends(self, q: int, stack) -> bool:
        return bool(self.accept[q]) and not len(stack)

    def matches(self, data: bytes, max_depth: int = MAX_DEPTH) -> bool:
        at = self.walk(self.start, (), data, max_depth)
        return at is not None and self.ends(*at)

    def table(self) -> np.ndarray:
        """uint8 [S * 769 + n_ret * 32]: the table as the calls take it (little-endian uint16 trans[S][256], uint16 ret[n_ret][16], uint8
        op[S][256], uint8 accept[S])."""
        return np.concatenate([np.ascontiguousarray(self.trans, dtype="<u2").view(np.uint8).reshape(-1),
                               np.ascontiguousarray(self.ret, dtype="<u2").view(np.uint8).reshape(-1),
                               np.ascontiguousarray(self.op, dtype=np.uint8).reshape(-1), self.accept])

    def shortest_completion(self, q: int, stack, max_depth: int = MAX_DEPTH) -> Optional[bytes]:
        """The fewest bytes from (q, stack) to an accepting configuration with an empty stack -- "close this document now" -- the lowest
        bytes first among equals; None where there is none.  Breadth first over configurations.  Completions that never push are looked
        for first (a push asks for a pop of its own, so in a bracket language none is shorter); only where there is none are pushes
        followed too."""
        for pushes in (False, True):
            first = (int(q), tuple(stack))
            seen, level = {first: None}, [first]
            while level:
                nxt = []
                for at in level:
                    if self.ends(*at):
                        out = bytearray()
                        while seen[at] is not None:
                            at, x = seen[at]
                            out.append(x)
                        return bytes(reversed(out))
                    row_t, row_o = self.trans[at[0]], self.op[at[0]]
                    for x in np.flatnonzero((row_t < self.n_states) | (row_o != 0)).tolist():
                        if not pushes and int(row_o[x]) & 0xF0 == PUSH:
                            continue
                        to = self.step(at[0], at[1], x, max_depth)
                        if to is not None and to not in seen:
                            seen[to] = (at, x)
                            nxt.append(to)
                level = nxt
                if pushes and len(seen) > 1 << 16:
                    break
        return None

    def __repr__(self) -> str:
        return "NestTable(n_states=%d, n_ret=%d, start=%d)" % (self.n_states, self.n_ret, self.start)


def from_dfa(dfa) -> NestTable:
    """The nest table of a splintr_amd.dfa.ByteDFA (or of (trans, accept)): every op zero, no ret row."""
    trans, accept = (dfa.trans, dfa.accept) if hasattr(dfa, "trans") else dfa
    trans = np.ascontiguousarray(trans, dtype=np.uint16)
    return NestTable(trans, np.zeros(trans.shape, dtype=np.uint8), np.zeros((0, 16), dtype=np.uint16), np.asarray(accept),
                     getattr(dfa, "start", 0))


# ---------------------------------------------------------------------------------------------- JSON
SYM_TOP, SYM_MEMBER, SYM_ELEMENT = 0, 1, 2
_WS = b" \t\n\r"
_HEX = b"0123456789abcdefABCDEF"
_DIGITS = b"0123456789"


class _Builder:
    """named states, byte -> (target, op)"""

    def __init__(self):
        self.rows, self.accepting = {}, set()

    def add(self, name, data, target, op=0):
        row = self.rows.setdefault(name, {})
        for x in data:
            assert x not in row, (name, x)
            row[x] = (target, op)

    def build(self, start, ret_names):
        # the reachable states, numbered breadth first from the start, bytes in order
        number, queue = {start: 0}, [start]
        for name in queue:
            targets = [t for _, (t, o) in sorted(self.rows.get(name, {}).items())]
            if any(o == POP for _, o in self.rows.get(name, {}).values()):
                targets += list(ret_names)
            for t in targets:
                if t is not None and t not in number:
                    number[t] = len(number)
                    queue.append(t)
        S = len(queue)
        trans = np.full((S, 256), DEAD, dtype=np.uint16)
        op = np.zeros((S, 256), dtype=np.uint8)
        for name, q in number.items():
            for x, (t, o) in self.rows.get(name, {}).items():
                trans[q, x] = 0 if o == POP else number[t]                       # (a pop: the ret row, there is one)
                op[q, x] = o
        ret = np.full((1, 16), DEAD, dtype=np.uint16)
        for y, name in enumerate(ret_names):
            if name in number:
                ret[0, y] = number[name]
        accept = np.array([1 if name in self.accepting else 0 for name in queue], dtype=np.uint8)
        return NestTable(trans, op, ret, accept, 0), number


def json_table(top: str = "value", ws: str = "json") -> NestTable:
    """The nest table of JSON: RFC 8259 as Python's json.loads reads it with NaN and Infinity refused.  Strings hold no raw byte below
    0x20, the escapes \\" \\\\ \\/ \\b \\f \\n \\r \\t \\uXXXX and only well-formed UTF-8 (no overlongs, no encoded surrogates, nothing
    above U+10FFFF); numbers are -?(0|[1-9][0-9]*)(\\.[0-9]+)?([eE][+-]?[0-9]+)?, ended by what follows them.  top: "value" (any JSON
    value), "object" or "array" (the document is one).  ws: "json" -- any run of space, tab, newline, carriage return wherever JSON
    allows it; "compact" -- at most one space after , and : and none elsewhere (both of json.dumps' usual separators); "none".  An
    opener pushes the kind of the context it stands in -- top, member value, element -- and one ret row serves every closer: the state
    says which container is open, the stack which one encloses it."""
    if top not in ("value", "object", "array"):
        raise ValueError('top must be "value", "object" or "array", not %r' % (top,))
    if ws not in ("json", "compact", "none"):
        raise ValueError('ws must be "json", "compact" or "none", not %r' % (ws,))
    b = _Builder()
    free_ws = _WS if ws == "json" else b""
    sym = {"T": SYM_TOP, "O": SYM_MEMBER, "A": SYM_ELEMENT}

    def string(p, leave):
        """a string behind its opening quote, states p + ...; the closing quote goes to `leave`"""
        s = p + "s"
        b.add(s, b'"', leave)
        b.add(s, b"\\", p + "esc")
        b.add(s, bytes(x for x in range(0x20, 0x80) if x not in b'"\\'), s)
        b.add(s, range(0xC2, 0xE0), p + "c1")
        b.add(s, b"\xe0", p + "e0")
        b.add(s, bytes([*range(0xE1, 0xED), 0xEE, 0xEF]), p + "c2")
        b.add(s, b"\xed", p + "ed")
        b.add(s, b"\xf0", p + "f0")
        b.add(s, range(0xF1, 0xF4), p + "c3")
        b.add(s, b"\xf4", p + "f4")
        b.add(p + "c1", range(0x80, 0xC0), s)
        b.add(p + "c2", range(0x80, 0xC0), p + "c1")
        b.add(p + "c3", range(0x80, 0xC0), p + "c2")
        b.add(p + "e0", range(0xA0, 0xC0), p + "c1")
        b.add(p + "ed", range(0x80, 0xA0), p + "c1")
        b.add(p + "f0", range(0x90, 0xC0), p + "c2")
        b.add(p + "f4", range(0x80, 0x90), p + "c2")
        b.add(p + "esc", b'"\\/bfnrt', s)
        b.add(p + "esc", b"u", p + "u1")
        for k in (1, 2, 3):
            b.add(p + "u%d" % k, _HEX, p + "u%d" % (k + 1))
        b.add(p + "u4", _HEX, s)

    def value_starts(state, c):
        """what may begin a value in context c"""
        b.add(state, b'"', c + "s")
        b.add(state, b"-", c + "neg")
        b.add(state, b"0", c + "zero")
        b.add(state, b"123456789", c + "int")
        for word in (b"true", b"false", b"null"):
            b.add(state, word[:1], c + word[:1].decode())
        b.add(state, b"{", "obj0", PUSH | sym[c])
        b.add(state, b"[", "arr0", PUSH | sym[c])

    def after(state, c):
        """what may follow a value in context c"""
        b.add(state, free_ws, c + "after")
        if c == "O":
            b.add(state, b",", "keyexp")
            b.add(state, b"}", None, POP)
        elif c == "A":
            b.add(state, b",", "Aval0")
            b.add(state, b"]", None, POP)
        else:
            b.accepting.add(state)

    for c in "TOA":
        # Xval0: behind , or : -- "compact" allows one space here; Xval: no space may follow any more
        b.add(c + "val", free_ws, c + "val")
        value_starts(c + "val", c)
        if ws == "compact" and c != "T":
            b.add(c + "val0", b" ", c + "val")
        else:
            b.add(c + "val0", free_ws, c + "val0")
        value_starts(c + "val0", c)
        string(c, c + "after")
        b.add(c + "neg", b"0", c + "zero")
        b.add(c + "neg", b"123456789", c + "int")
        b.add(c + "int", _DIGITS, c + "int")
        for done in ("zero", "int"):
            b.add(c + done, b".", c + "frac0")
            b.add(c + done, b"eE", c + "exp0")
        b.add(c + "frac0", _DIGITS, c + "frac")
        b.add(c + "frac", _DIGITS, c + "frac")
        b.add(c + "frac", b"eE", c + "exp0")
        b.add(c + "exp0", b"+-", c + "exps")
        b.add(c + "exp0", _DIGITS, c + "exp")
        b.add(c + "exps", _DIGITS, c + "exp")
        b.add(c + "exp", _DIGITS, c + "exp")
        for word in (b"true", b"false", b"null"):
            for k in range(1, len(word)):
                b.add(c + word[:k].decode(), word[k:k + 1], c + (word[:k + 1].decode() if k + 1 < len(word) else "after"))
        for done in ("zero", "int", "frac", "exp", "after"):                     # a number is ended by what follows it
            after(c + done, c)
    b.add("obj0", free_ws, "obj0")
    b.add("obj0", b'"', "Ks")
    b.add("obj0", b"}", None, POP)
    if ws == "compact":
        b.add("keyexp", b" ", "keyexp1")
        b.add("keyexp1", b'"', "Ks")
    else:
        b.add("keyexp", free_ws, "keyexp")
    b.add("keyexp", b'"', "Ks")
    string("K", "colon")
    b.add("colon", free_ws, "colon")
    b.add("colon", b":", "Oval0")
    b.add("arr0", free_ws, "arr0")
    value_starts("arr0", "A")
    b.add("arr0", b"]", None, POP)
    if top == "value":
        start = "Tval"
    else:
        start = "start"
        b.add(start, free_ws, start)
        b.add(start, b"{" if top == "object" else b"[", "obj0" if top == "object" else "arr0", PUSH | SYM_TOP)
    table, _ = b.build(start, ["Tafter", "Oafter", "Aafter"])
    return table
