"""The two oracles of spl_stream_decode_device over an {id: bytes} table (tests/decode_ref.Table), one decoder per sequence:

hold mode     splintr_amd.streaming.StreamingDecoder (the reference's decoder, step for step): the text it emits and its pending_bytes
replace mode  codecs.getincrementaldecoder("utf-8")("replace"), fed with final=False

and helpers to read the device's state word."""
import codecs
import functools
import itertools

import numpy as np

from splintr_amd.streaming import StreamingDecoder

REPLACE, FINAL_ALL = 1, 2
FFFD = b"\xef\xbf\xbd"


# ------------------------------------------------------------------------------------------ the test vocabulary and the exhaustive strings
ALPHABET = [0x41, 0x80, 0xBF, 0xC0, 0xC2, 0xE0, 0xA0, 0xED, 0xE1, 0xF0, 0x90, 0xF4, 0x8F, 0xF5, 0xFF]
CH2, CH3, CH4 = "é".encode(), "你".encode(), "😀".encode()
KEY4, KEY2, LIT3, SPECIAL, FAR = 256, 302, 300, 301, 5_000_000       # ids of byte_table beyond its 256 single bytes
UNKNOWN = (257, 299, 303, 310, 311, 4_999_999, 0xFFFFFFFF)
MAX_ID = 310


def byte_table():
    """id i < 256: the single byte i.  KEY4: a 300-byte key of 75 four-byte characters ROTATED by one byte (it begins with the last three
    bytes of one and ends with the lead of the next); KEY2: a 300-byte key of 150 two-byte characters; LIT3: a special token's 255-byte
    literal of 85 three-byte characters; SPECIAL, FAR: short special tokens inside and beyond the dense id range."""
    from decode_ref import Table
    toks = {i: bytes([i]) for i in range(256)}
    toks[KEY4] = (CH4 * 76)[1:301]
    toks[KEY2] = CH2 * 150
    toks[LIT3] = CH3 * 85
    toks[SPECIAL] = b"<|s|>"
    toks[FAR] = b"<far>"
    assert len(toks[KEY4]) == 300 and len(toks[LIT3]) == 255
    return Table(toks, special_only={LIT3, SPECIAL, FAR})


_strings = None


def alphabet_strings():
    """every string of length 1 .. 4 over ALPHABET (54 240 of them), shortest first"""
    global _strings
    if _strings is None:
        import itertools
        _strings = [bytes(s) for n in range(1, 5) for s in itertools.product(ALPHABET, repeat=n)]
        assert len(_strings) == 54240
    return _strings


def rows_of(strings, K=4, dtype=np.uint32):
    """the strings as rows of single-byte ids [B, K] and their lengths"""
    rows = np.zeros((len(strings), K), dtype=dtype)
    lens = np.zeros(len(strings), dtype=np.int32)
    for b, s in enumerate(strings):
        rows[b, :len(s)] = list(s)
        lens[b] = len(s)
    return rows, lens


def straddle_rows():
    """Long tokens behind 0 .. 11 ASCII bytes, so that a 2-, 3- and 4-byte character straddles every multiple of every chunk size used: a row
    is [shift x 'a'] [the lead of CH4] KEY4 [the rest of CH4] KEY2 LIT3 'z' [the first two bytes of CH3]; and the same with the 300-byte key
    cut off from its lead by an unknown id, a far special and a skipped one."""
    rows = []
    for shift in range(12):
        rows.append([0x61] * shift + [CH4[0], KEY4] + list(CH4[1:]) + [KEY2, LIT3, 0x7A] + list(CH3[:2]))
        rows.append([0x61] * shift + [CH4[0], UNKNOWN[0], KEY4, FAR, SPECIAL] + list(CH4[1:]) + [LIT3, KEY2])
        rows.append([0x61] * shift + [KEY4, KEY4, 0x41])          # begins with continuation bytes
    K = max(len(r) for r in rows)
    lens = np.array([len(r) for r in rows], dtype=np.int32)
    return np.array([r + [0x41] * (K - len(r)) for r in rows], dtype=np.int64), lens          # (the padding would decode to something)


_memo = {}


def alphabet_oracle(replace, way):
    """The oracle's answer for every alphabet string, computed once and shared (tests must not change it): way "steps": one byte per step,
    four steps and a final one -> list of five Batch.step results; "whole": all bytes in one step, then final -> two results."""
    key = (bool(replace), way)
    if key not in _memo:
        strings = alphabet_strings()
        rows, lens = rows_of(strings)
        bt = Batch(byte_table(), len(strings), 0, replace)
        res = []
        if way == "steps":
            for k in range(4):
                res.append(bt.step(rows[:, k:k + 1], (lens > k).astype(np.int32)))
        else:
            res.append(bt.step(rows, lens))
        res.append(bt.step(rows[:, :1], np.zeros(len(strings), dtype=np.int32), np.ones(len(strings), dtype=np.uint8)))
        _memo[key] = res
    return _memo[key]


# ------------------------------------------------------------------------------------------ the state word
def st_count(s):
    return (int(s) >> 24) & 3


def st_stalled(s):
    return (int(s) >> 26) & 1


def st_held(s):
    return int(s) >> 32


def st_pending_bytes(s):
    """what the reference's pending_bytes is: the count where the sequence is not stalled, held where it is"""
    return st_held(s) if st_stalled(s) else st_count(s)


def st_pending(s):
    return bytes((int(s) >> (8 * i)) & 0xFF for i in range(st_count(s)))


def st_well_formed(s):
    """every bit the header does not name is 0, pending bytes beyond the count are 0, a stalled word has no pending bytes"""
    s = int(s)
    if s & ~(0xFFFFFFFF07FFFFFF):
        return False
    if st_stalled(s):
        return (s & 0x3FFFFFF) == 0
    return st_held(s) == 0 and (s & 0xFFFFFF) >> (8 * st_count(s)) == 0


def slot_bytes(tab, v, flags):
    return tab.span(v, flags)


# ------------------------------------------------------------------------------------------ one sequence
@functools.lru_cache(maxsize=None)
def _can_complete(buf):
    """some continuation makes the (non-empty, invalid) buffer ONE valid character: it is the beginning of a character by Unicode's table.
    Asked of the decoder itself, not of its error message: the candidates are the edges of every second-byte range of the table."""
    if not 1 <= len(buf) <= 3:
        return False
    edges = (0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF)
    for n in range(1, 4 - len(buf) + 1):
        for tail in itertools.product(edges, repeat=n):
            try:
                if len((buf + bytes(tail)).decode("utf-8")) == 1:
                    return True
            except UnicodeDecodeError:
                pass
    return False


class Hold:
    def __init__(self, tab, flags=0):
        self.tab, self.flags = tab, flags
        self.dec = StreamingDecoder(lambda t: None)       # (fed with bytes below, not through the lookup)

    def _unfinished(self):
        """the buffer is the well-formed beginning of one character (what the device keeps as pending)"""
        return _can_complete(bytes(self.dec._buf))

    @property
    def stalled(self):
        return bool(self.dec._buf) and not self._unfinished()

    @property
    def pending_bytes(self):
        return self.dec.pending_bytes

    def step(self, ids, final=False):
        """-> the bytes that leave for these ids (a list of id VALUES, already cut to the row's valid entries)"""
        for v in ids:
            self.dec._buf += slot_bytes(self.tab, v, self.flags)
        out = self.dec._extract()
        out = out.encode("utf-8") if out else b""
        if final and self.dec._buf and not self.stalled:
            out += self.dec.flush().encode("utf-8")
            assert out.endswith(FFFD)
        return out


class Replace:
    def __init__(self, tab, flags=0):
        self.tab, self.flags = tab, flags
        self.dec = codecs.getincrementaldecoder("utf-8")("replace")

    stalled = False

    @property
    def pending_bytes(self):
        return len(self.dec.getstate()[0])

    def step(self, ids, final=False):
        chunk = b"".join(slot_bytes(self.tab, v, self.flags) for v in ids)
        out = self.dec.decode(chunk, final=False)
        held = self.dec.getstate()[0]
        if held and not _can_complete(held):
            # Some CPython versions (3.10 among them) keep ED A0 .. ED BF (the beginning of an encoded surrogate) until a third byte arrives and replaces the
            # two bytes only then; by the table the second byte does not conform to ED, so the two units are due NOW -- which is what the
            # same decoder answers once it is told that nothing follows.  Only the step in which the text leaves differs, never the text.
            assert len(held) == 2 and held[0] == 0xED and held[1] >= 0xA0, held
            out += self.dec.decode(b"", final=True)
            self.dec.reset()
        if final:
            out += self.dec.decode(b"", final=True)
            self.dec.reset()
        return out.encode("utf-8")


def make(tab, flags=0, replace=False):
    return (Replace if replace else Hold)(tab, flags)


# ------------------------------------------------------------------------------------------ a batch
class Batch:
    """B decoders; step(rows [B, K], lengths or None, final [B] or None) -> (bytes per sequence, pending_bytes, stalled)"""

    def __init__(self, tab, n, flags=0, replace=False):
        self.decs = [make(tab, flags, replace) for _ in range(n)]

    def step(self, rows, lengths=None, final=None):
        rows = np.asarray(rows)
        K = rows.shape[1]
        outs = []
        for b, d in enumerate(self.decs):
            n = K if lengths is None else min(max(int(lengths[b]), 0), K)
            outs.append(d.step([int(v) for v in rows[b, :n]], bool(final[b]) if final is not None else False))
        return outs, [d.pending_bytes for d in self.decs], [int(d.stalled) for d in self.decs]


def check_step(tag, got_bytes, got_off, got_state, want):
    """a device (or simulated) step against Batch.step's result"""
    outs, pend, stalled = want
    off = [int(x) for x in got_off]
    assert off[0] == 0 and len(off) == len(outs) + 1, tag
    for b, w in enumerate(outs):
        g = got_bytes[off[b]:off[b + 1]]
        assert g == w, (tag, b, g, w)
        s = int(got_state[b])
        assert st_well_formed(s), (tag, b, hex(s))
        assert st_stalled(s) == stalled[b], (tag, b, hex(s), stalled[b])
        assert st_pending_bytes(s) == pend[b], (tag, b, hex(s), pend[b])
