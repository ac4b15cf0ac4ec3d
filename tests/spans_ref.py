"""Pure-Python statement of spl_token_spans_device's contract (include/splintr_hip.h), for the tests: plain loops over decode_ref.Table,
written from the rule -- per slot len / nch / cont, per document the running sums, the tiktoken start adjustment, (0, 0) for a slot
of no document, int32 saturation.  Slow and obvious."""
import numpy as np

from decode_ref import PAD_LEFT

INT32_MAX = (1 << 31) - 1


def slot_values(b):
    """(len, nch, cont) of a slot's decoded bytes"""
    nch = sum(1 for x in b if (x & 0xC0) != 0x80)
    cont = 1 if b and (b[0] & 0xC0) == 0x80 else 0
    return len(b), nch, cont


def _sat(v, i64):
    return v if i64 else min(v, INT32_MAX)


def _spans(tab, ids, docs, slots, flags, i64, length_of=None):
    """docs: per document the list of (slot, valid); slots of no document keep (0, 0).  length_of: a stand-in for len(bytes) (the
    saturation tests use lengths no byte string of the table has)."""
    dt = np.int64 if i64 else np.int32
    bspan = np.zeros((slots, 2), dtype=dt)
    cspan = np.zeros((slots, 2), dtype=dt)
    boff, coff = [0], [0]
    gb = gc = 0
    for doc in docs:
        bs = cs = 0
        for i, valid in doc:
            b = tab.span(ids[i], flags) if valid else b""
            ln, nch, cont = slot_values(b)
            if length_of is not None and valid:
                ln, nch, cont = length_of(int(ids[i]), ln, nch, cont)
            bspan[i] = (_sat(bs, i64), _sat(bs + ln, i64))
            cspan[i] = (_sat(cs - (1 if cont and cs > 0 else 0), i64), _sat(cs + nch, i64))
            bs += ln
            cs += nch
        gb += bs
        gc += cs
        boff.append(gb)
        coff.append(gc)
    return bspan, cspan, np.array(boff, dtype=np.uint64), np.array(coff, dtype=np.uint64)


def spans_csr(tab, ids, ids_off, n_ids_cap, flags=0, i64=False, length_of=None):
    """CSR mode: document d is the slots [off[d], off[d + 1]) with every offset clamped to n_ids_cap; off[0] == 0."""
    assert not flags & PAD_LEFT
    off = [min(int(x), int(n_ids_cap)) for x in ids_off]
    assert off[0] == 0
    docs = [[(i, True) for i in range(off[d], off[d + 1])] for d in range(len(off) - 1)]
    return _spans(tab, ids, docs, int(n_ids_cap), flags, i64, length_of)


def spans_rows(tab, rows, lengths=None, flags=0, i64=False):
    """rows mode: document r is row r; with lengths its first (PAD_LEFT: last) clamp(lengths[r], 0, row_len) entries are valid, the
    others are zero-length slots of the row"""
    rows = np.asarray(rows)
    n, L = rows.shape
    docs = []
    for r in range(n):
        k = L if lengths is None else max(0, min(int(lengths[r]), L))
        valid = range(L - k, L) if flags & PAD_LEFT else range(k)
        docs.append([(r * L + c, c in valid) for c in range(L)])
    return _spans(tab, rows.reshape(-1), docs, n * L, flags, i64)


def char_starts(byte_strings):
    """tiktoken's decode_with_offsets over one document's token byte strings -> the character start of every token"""
    out, cs = [], 0
    for b in byte_strings:
        ln, nch, cont = slot_values(b)
        out.append(cs - (1 if cont and cs > 0 else 0))
        cs += nch
    return out
