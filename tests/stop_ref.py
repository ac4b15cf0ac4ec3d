"""The oracle of spl_stop_match_device: the WHOLE-TEXT definition of include/splintr_hip.h, with bytes.endswith / startswith and nothing
incremental.  Per sequence, T is every byte fed so far and S the stops its mask selects:

  hit      the smallest end e such that some s of S is a suffix of T[:e]; of the stops ending there the longest wins (start p), of equal
           strings the lowest slot; released = T[:p] (include: T[:e]); the sequence is stopped, T counts as T[:e] from then on
  no hit   released = T[:|T| - h], h = the longest suffix of T that is a PROPER prefix of some s of S
  final    (no hit) the held bytes leave too; the text is closed: what is fed later is a new text, `released` goes on counting

A Seq answers every call from the whole text of its open segment; what a call emits is the released text now less the released text before."""
import functools

import numpy as np

SLOTS, MAX_LEN, TABLE_BYTES, WORDS, TAIL_MAX = 64, 64, 64 * 64 + 64, 10, 63
INCLUDE, FINAL_ALL = 1, 2


def table(stops, lens=None):
    """stops: list (slot = index) of bytes / str / None -> uint8 [TABLE_BYTES] as the device lays it out; lens overrides the length bytes
    ({slot: value}: what a test needs for a length of 0 or 65)."""
    t = np.zeros(TABLE_BYTES, dtype=np.uint8)
    assert len(stops) <= SLOTS
    for s, x in enumerate(stops):
        if x is None:
            continue
        b = x.encode("utf-8") if isinstance(x, str) else bytes(x)
        assert 1 <= len(b) <= MAX_LEN
        t[MAX_LEN * s:MAX_LEN * s + len(b)] = np.frombuffer(b, dtype=np.uint8)
        t[SLOTS * MAX_LEN + s] = len(b)
    for s, v in (lens or {}).items():
        t[SLOTS * MAX_LEN + s] = v
    return t


def live_stops(tab, mask=None):
    """[(slot, bytes)] in rising slot order: the slots of the mask (None: all) whose length is 1 .. 64"""
    out = []
    for s in range(SLOTS):
        n = int(tab[SLOTS * MAX_LEN + s])
        if 1 <= n <= MAX_LEN and (mask is None or (int(mask) >> s) & 1):
            out.append((s, bytes(tab[MAX_LEN * s:MAX_LEN * s + n])))
    return out


def first_hit(T, stops):
    """(e, p, slot) or None"""
    return _first_hit(bytes(T), tuple(stops))


@functools.lru_cache(maxsize=1 << 20)
def _first_hit(T, stops):
    for e in range(1, len(T) + 1):
        head, best = T[:e], None
        for slot, s in stops:                                  # (rising slots: of equal strings the first stays)
            if head.endswith(s) and (best is None or len(s) > len(best[1])):
                best = (slot, s)
        if best is not None:
            return e, e - len(best[1]), best[0]
    return None


def held(T, stops):
    return _held(bytes(T), tuple(stops))


@functools.lru_cache(maxsize=1 << 20)
def _held(T, stops):
    for k in range(min(len(T), TAIL_MAX), 0, -1):
        suf = T[len(T) - k:]
        if any(len(s) > k and s.startswith(suf) for _, s in stops):
            return k
    return 0


class Seq:
    """One sequence against the stops `stops` ([(slot, bytes)], as live_stops gives them)."""

    def __init__(self, stops, include=False):
        self.stops, self.include = stops, include
        self.closed = 0            # bytes of the closed texts in front of the open one
        self.T = b""               # the open text
        self.hit = -1
        self.released = 0          # of closed + T
        self.h = 0

    def feed(self, data=b"", final=False):
        """-> the bytes that leave now"""
        if self.hit >= 0:
            return b""
        before = self.released - self.closed                   # (within T: a closed text is released whole)
        self.T += bytes(data)
        found = first_hit(self.T, self.stops)
        if found is not None:
            e, p, self.hit = found
            self.T = self.T[:e]
            cut, self.h = (e if self.include else p), 0
        elif final:
            cut, self.h = len(self.T), 0
        else:
            self.h = held(self.T, self.stops)
            cut = len(self.T) - self.h
        assert cut >= before, "the released text shrank"
        out = self.T[before:cut]
        self.released = self.closed + cut
        if final and found is None:
            self.closed += len(self.T)
            self.T = b""
        return out

    def row(self):
        """the state row: uint64 [10]"""
        tail = self.T[-TAIL_MAX:] if self.T else b""
        w0 = len(tail) | (self.h << 8) | ((1 << 16) | (self.hit << 24) if self.hit >= 0 else 0)
        return np.frombuffer(w0.to_bytes(8, "little") + self.released.to_bytes(8, "little") + tail + bytes(64 - len(tail)), dtype="<u8")


def run_calls(seqs, calls):
    """seqs: [Seq]; calls: per call a list of (data, final) per sequence -> per call (bytes, out_off [B + 1], hit [B], rows [B, 10])"""
    res = []
    for call in calls:
        outs = [q.feed(d, f) for q, (d, f) in zip(seqs, call)]
        off = np.concatenate([[0], np.cumsum([len(o) for o in outs])]).astype(np.uint64)
        rows = np.stack([q.row() for q in seqs]) if seqs else np.zeros((0, WORDS), dtype=np.uint64)
        res.append((b"".join(outs), off, np.array([q.hit for q in seqs], dtype=np.int32), rows))
    return res


def csr(datas):
    """[bytes] -> (uint8 array, uint64 offsets [B + 1])"""
    off = np.concatenate([[0], np.cumsum([len(d) for d in datas])]).astype(np.uint64)
    return np.frombuffer(b"".join(datas), dtype=np.uint8).copy(), off
