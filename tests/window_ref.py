"""What spl_window_device must produce, restated with plain loops over numpy arrays (TEST TOOL; the analogue of collate_ref.py).

Written from the semantics in include/splintr_hip.h, not from the kernels: a document's windows are cut from the list of its ids, one
after the other, until the list is used up.  Values are kept as uint64 holding the 32-bit pattern, so an int64 output must EQUAL them
(zero extension) and an int32 output must equal their low 32 bits.
"""
import numpy as np

from collate_ref import BOS, EOS, I64, KEEP_TAIL, PAD_LEFT, csr, n_special   # noqa: F401  (re-exported for the tests)


def doc_windows(toks, B, overlap):
    """[(start, body)] of one document: windows of at most B ids that overlap by `overlap`; at least one, also for no ids at all"""
    assert B >= 1 and 0 <= overlap < B
    step = B - overlap
    out, start = [], 0
    while True:
        out.append((start, toks[start:start + B]))
        if start + B >= len(toks):               # this window reaches the document's end: it is the last one
            return out
        start += step


def window_ref(ids, off, L, flags, overlap, pad_id, bos_id=0, eos_id=0):
    """-> rows uint64 [n_rows, L], mask uint8 [n_rows, L], lengths int32 [n_rows], doc int32 [n_rows], start int64 [n_rows],
    row_off uint64 [n_docs + 1]"""
    n_docs = len(off) - 1
    k = n_special(flags)
    assert L > k and not flags & KEEP_TAIL
    rows, mask, lens, docs, starts, row_off = [], [], [], [], [], [0]
    for d in range(n_docs):
        toks = [int(x) for x in ids[int(off[d]):int(off[d + 1])]]
        for start, body in doc_windows(toks, L - k, overlap):
            row = ([bos_id] if flags & BOS else []) + body + ([eos_id] if flags & EOS else [])
            fill = [pad_id] * (L - len(row))
            rows.append(fill + row if flags & PAD_LEFT else row + fill)
            mask.append([0] * len(fill) + [1] * len(row) if flags & PAD_LEFT else [1] * len(row) + [0] * len(fill))
            lens.append(len(row))
            docs.append(d)
            starts.append(start)
        row_off.append(len(rows))
    return (np.array(rows, dtype=np.uint64).reshape(len(rows), L), np.array(mask, dtype=np.uint8).reshape(len(rows), L),
            np.array(lens, dtype=np.int32), np.array(docs, dtype=np.int32), np.array(starts, dtype=np.int64),
            np.array(row_off, dtype=np.uint64))


def edge_lengths(B, step):
    """the document lengths at which the number of windows changes, and their neighbours"""
    return sorted({max(0, x) for x in (0, 1, B - 1, B, B + 1, B + step - 1, B + step, B + step + 1)})


def overlaps(B):
    return sorted({0, min(1, B - 1), B - 1})
