"""The rule of spl_utf8_mask_device in plain Python (TEST TOOL): which ids may follow the pending bytes of a streaming decoder so that its
text stays well-formed UTF-8.  prefix_valid states Unicode's Table 3-7 byte by byte; tests/test_utf8mask_cpu.py pins it against Python's own
incremental decoder and against the hold-mode decoders of splintr_amd.streaming.  A toy vocabulary with every edge of the table, the
states (one representative and both boundaries of each of the eight classes, and a stalled one), and a judge for whole shipped
vocabularies (Python's decoder behind a representative of every class) live here too."""
import codecs

import numpy as np

STALLED = 1 << 26
N_CLASSES = 8


def _second(lead):
    """the range of the byte behind `lead`"""
    return {0xE0: (0xA0, 0xBF), 0xED: (0x80, 0x9F), 0xF0: (0x90, 0xBF), 0xF4: (0x80, 0x8F)}.get(lead, (0x80, 0xBF))


def _want(lead):
    return 1 if 0xC2 <= lead <= 0xDF else 2 if 0xE0 <= lead <= 0xEF else 3 if 0xF0 <= lead <= 0xF4 else 0


def prefix_valid(b):
    """b is well-formed UTF-8, optionally followed by the well-formed beginning of one character that reaches the end"""
    i, n = 0, len(b)
    while i < n:
        x = b[i]
        if x < 0x80:
            i += 1
            continue
        w = _want(x)
        if not w:
            return False
        for k in range(1, w + 1):
            if i + k >= n:
                return True                       # the beginning of a character reaches the end
            lo, hi = _second(x) if k == 1 else (0x80, 0xBF)
            if not lo <= b[i + k] <= hi:
                return False
        i += w + 1
    return True


def is_beginning(p):
    """p is the well-formed beginning of ONE character, unfinished (what a decoder keeps pending), or empty"""
    return len(p) == 0 or (len(p) <= 3 and _want(p[0]) >= len(p) and prefix_valid(p))


def pending_class(p):
    """0 start; 1, 2, 3 that many continuation bytes of any value owed; 4, 5, 6, 7 behind E0, ED, F0, F4"""
    assert is_beginning(p)
    if not p:
        return 0
    if len(p) == 1 and p[0] in (0xE0, 0xED, 0xF0, 0xF4):
        return {0xE0: 4, 0xED: 5, 0xF0: 6, 0xF4: 7}[p[0]]
    return _want(p[0]) - (len(p) - 1)


# one pending string per class (class 0: none)
CLASS_REPS = [b"", b"\xc3", b"\xe1", b"\xf1", b"\xe0", b"\xed", b"\xf0", b"\xf4"]


def state_word(p=b"", stalled=False, held=0):
    """the stream decoder's state word (include/splintr_hip.h): pending bytes, their count, stalled, held"""
    if stalled:
        return STALLED | (held << 32)
    return int.from_bytes(p, "little") | (len(p) << 24)


def emitted(vocab, specials, t, skip):
    """what the streaming decode emits for id t (None: the id is not known)"""
    if t in vocab:
        return vocab[t]
    if t in specials:
        return b"" if skip else specials[t]
    return None


def allowed(vocab, specials, p, skip=False):
    """the ids whose bit is 1 behind the pending bytes p"""
    out = set()
    for t in set(vocab) | set(specials):
        e = emitted(vocab, specials, t, skip)
        if prefix_valid(p + e):
            out.add(t)
    return out


def mask_row(vocab, specials, word, skip, n_words):
    """(row uint32 [n_words], live) for one state word"""
    if word & STALLED:
        return np.full(n_words, 0xFFFFFFFF, dtype=np.uint32), 0
    n = (word >> 24) & 3
    p = (word & 0xFFFFFF).to_bytes(3, "little")[:n]
    bits = np.zeros(n_words * 32, dtype=np.uint8)
    for t in allowed(vocab, specials, p, skip):
        bits[t] = 1
    return np.packbits(bits, bitorder="little").view(np.uint32).copy(), 1


def masks(vocab, specials, words, skip, n_words):
    rows = [mask_row(vocab, specials, int(w), skip, n_words) for w in words]
    m = np.stack([r for r, _ in rows]) if rows else np.zeros((0, n_words), dtype=np.uint32)
    return m, np.array([l for _, l in rows], dtype=np.uint8)


# ---------------------------------------------------------------------------------------------- the toy vocabulary and the states
def toy(with_empty=True):
    """(vocab {id: bytes}, specials {id: bytes}): every single byte; every lead with its boundary second bytes; tokens that begin with 1, 2
    and 3 continuation bytes; tokens that end in 1 to 3 bytes of an unfinished character; a long valid token with one bad byte late; an
    empty token; a special id below and one above the largest vocabulary id; holes.  with_empty False: the vocabulary as the library's
    loader keeps it -- an empty key can never match a chunk and is dropped, so its id is a hole (toy_empty_id() names it)."""
    toks = [bytes([b]) for b in range(256)]
    toks += [b"\xc0\x80", b"\xc1\xbf", b"\xc2\x80", b"\xc2\x7f", b"\xdf\xbf", b"\xdf\xc0", b"\xe0\x9f", b"\xe0\xa0", b"\xe0\xa0\x80", b"\xe0\x9f\x80",
             b"\xed\x9f", b"\xed\xa0", b"\xed\x9f\xbf", b"\xed\xa0\x80", b"\xf0\x8f", b"\xf0\x90", b"\xf0\x90\x80\x80", b"\xf0\x8f\x80\x80",
             b"\xf4\x8f", b"\xf4\x90", b"\xf4\x8f\xbf\xbf", b"\xf4\x90\x80\x80", b"\xf5\x80", b"\xf5"[:1] + b"a"]
    toks += [b"\x80a", b"\x9f\xc3", b"\xa0a", b"\xbfa", b"\x8f\x80a", b"\x90\x80a", b"\x80\x80a", b"\xbf\xbf\xc3\xa9", b"\x80\x80\x80a",
             b"\x90\xbf\xbfz", b"\x8f\xbf\xbf", b"\x80\x80\x80\x80", b"\xa0\x80\xe2\x82", b"\x9f\xbf\xf0\x9f\x98"]
    toks += [b"a\xc3", b"ab\xe2", b"ab\xe2\x82", b"abc\xf0", b"abc\xf0\x9f", b"abc\xf0\x9f\x98", b"\xc3\xa9\xe0", b"\xe2\x82\xac\xed", b"z\xf4", b"z\xf0"]
    long_ok = "héllo wörld €uro 😀 ".encode() * 3
    toks += [long_ok, long_ok[:40] + b"\xff" + long_ok[41:], long_ok + b"\xe2\x82", long_ok[1:3] + long_ok, b"\xa9" + long_ok, b"\xa9" + long_ok[:50] + b"\xc0"]
    vocab, i = {}, 0
    for k, b in enumerate(toks):
        if k % 37 == 36:
            i += 1 + k % 3                         # holes
        vocab[i] = b
        i += 1
    empty = i + 2
    if with_empty:
        vocab[empty] = b""                         # an empty token, holes on both sides
    vocab[empty + 3] = b"tail"
    specials = {empty + 1: b"<|low|>", empty + 40: b"<|high|>", empty + 70: "<|\u00e9|>".encode()}
    return vocab, specials


def toy_empty_id():
    return max(toy()[0]) - 3


def toy_states():
    """(label, state word): one representative and both boundaries of each of the eight classes, and stalled words"""
    ps = [b"",
          b"\xc2", b"\xc3", b"\xdf", b"\xe1\x80", b"\xe0\xa0", b"\xed\x9f", b"\xef\xbf", b"\xf0\x90\x80", b"\xf1\x80\x80", b"\xf4\x8f\xbf",
          b"\xe1", b"\xe2", b"\xec", b"\xee", b"\xef", b"\xf0\x90", b"\xf0\xbf", b"\xf1\x80", b"\xf3\xbf", b"\xf4\x80", b"\xf4\x8f",
          b"\xf1", b"\xf2", b"\xf3",
          b"\xe0", b"\xed", b"\xf0", b"\xf4"]
    out = [(p.hex() or "start", state_word(p)) for p in ps]
    out += [("stalled", state_word(stalled=True, held=5)), ("stalled-max", state_word(stalled=True, held=0xFFFFFFFF))]
    return out


# ---------------------------------------------------------------------------------------------- whole vocabularies
def _py_valid(b):
    """Python's incremental decoder as the judge of prefix validity: it raises at the first byte the table forbids; what it still holds
    at the end must be the beginning of a character (some CPython versions hold ED A0 until a third byte arrives)"""
    dec = codecs.getincrementaldecoder("utf-8")("strict")
    try:
        dec.decode(b, False)
    except UnicodeDecodeError:
        return False
    return is_beginning(dec.getstate()[0])


def class_table(tokens, n_words):
    """tokens [(id, bytes)] -> uint32 [8, n_words]: row c holds the ids allowed behind a pending string of class c.  A pending string owes
    a continuation byte, so only the (few thousand) tokens that begin with one, and the empty ones, can follow it: they are judged behind a
    representative of every class, all others from the start alone."""
    bits = np.zeros((N_CLASSES, n_words * 32), dtype=np.uint8)
    for t, b in tokens:
        if b and not 0x80 <= b[0] <= 0xBF:
            bits[0, t] = _py_valid(b)
        else:
            for c in range(N_CLASSES):
                bits[c, t] = _py_valid(CLASS_REPS[c] + b)
    return np.packbits(bits, axis=1, bitorder="little").view(np.uint32).reshape(N_CLASSES, n_words).copy()
