"""The reference of spl_seqpack_device: plain loops written from include/splintr_hip.h (TEST TOOL; numpy only, no GPU).

plan()  where every sequence goes -- the two placement strategies, word for word.
pack()  every output of the call from the plan.
"""
from collections import namedtuple

import numpy as np

NEXT_FIT, BEST_FIT_DECREASING = 0, 1
STRATEGIES = {"next_fit": NEXT_FIT, "best_fit_decreasing": BEST_FIT_DECREASING}

Plan = namedtuple("Plan", "rows place clen cut")          # rows: list of lists of sequence indices; place [n, 2]; clipped lengths; cut flags
Packed = namedtuple("Packed", "input_ids labels bytes attention_mask position_ids seq_ids seq_place row_fill cu_seqlens n status")


def clip(lengths, row_len):
    """(clipped lengths, cut flags): min(len, row_len)"""
    lengths = [int(x) for x in lengths]
    return [min(x, row_len) for x in lengths], [x > row_len for x in lengths]


def plan(lengths, row_len, strategy):
    clen, cut = clip(lengths, row_len)
    n = len(clen)
    rows, place = [], [(-1, -1)] * n
    if strategy in (NEXT_FIT, "next_fit"):
        f = 0
        for i, l in enumerate(clen):
            if l == 0:
                continue
            if not rows or f + l > row_len:
                rows.append([])
                f = 0
            place[i] = (len(rows) - 1, f)
            rows[-1].append(i)
            f += l
    elif strategy in (BEST_FIT_DECREASING, "best_fit_decreasing"):
        order = sorted((i for i in range(n) if clen[i]), key=lambda i: (-clen[i], i))
        resid, stamp, tick = [], [], 0                    # per row: what is left of it, and when it reached that residual
        has_room = []                                     # (the rows with a residual above 0: a full row is never looked at again)
        for i in order:
            l = clen[i]
            best = -1
            for r in has_room:
                if resid[r] >= l and (best < 0 or resid[r] < resid[best] or (resid[r] == resid[best] and stamp[r] > stamp[best])):
                    best = r
            if best < 0:
                rows.append([])
                resid.append(row_len)
                stamp.append(0)
                best = len(rows) - 1
                has_room.append(best)
            place[i] = (best, row_len - resid[best])
            rows[best].append(i)
            resid[best] -= l
            tick += 1
            stamp[best] = tick
            if resid[best] == 0:
                has_room.remove(best)
    else:
        raise ValueError(strategy)
    return Plan(rows, np.array(place, dtype=np.int32).reshape(n, 2), clen, cut)


def pack(seqs, row_len, strategy, *, max_rows=None, pad_id=0, ignore_index=-100, labels=None, byte_arrays=(None,) * 4, fills=(0, 0, 0, 0),
         keep_tail=False, mask_first=True, bad=()):
    """seqs: a list of id lists (what the input holds of every sequence, before clipping); labels / byte_arrays[k]: lists in the same
    shape or None; bad: indices of sequences the device reports (status 1) and treats as empty.  -> Packed, numpy arrays; ids and labels
    int64 (labels: ids zero-extended, ignore_index as the number it is)."""
    n = len(seqs)
    max_rows = n if max_rows is None else max_rows
    lengths = [0 if i in bad else len(s) for i, s in enumerate(seqs)]
    p = plan(lengths, row_len, strategy)
    R, L = max_rows, row_len
    ids = np.full((R, L), pad_id, dtype=np.int64)
    lab = None if labels is None else np.full((R, L), ignore_index, dtype=np.int64)
    byt = [None if a is None else np.full((R, L), fills[k], dtype=np.uint8) for k, a in enumerate(byte_arrays)]
    mask = np.zeros((R, L), dtype=np.uint8)
    pos = np.zeros((R, L), dtype=np.int32)
    sid = np.full((R, L), -1, dtype=np.int32)
    fill = np.zeros(R, dtype=np.int32)
    cu = []
    for r, row in enumerate(p.rows[:R]):
        for i in row:
            c, l = int(p.place[i, 1]), p.clen[i]
            first = len(seqs[i]) - l if keep_tail else 0
            ids[r, c:c + l] = seqs[i][first:first + l]
            if lab is not None:
                lab[r, c:c + l] = labels[i][first:first + l]
                if mask_first:
                    lab[r, c] = ignore_index
            for k, a in enumerate(byte_arrays):
                if a is not None:
                    byt[k][r, c:c + l] = a[i][first:first + l]
            mask[r, c:c + l] = 1
            pos[r, c:c + l] = np.arange(l)
            sid[r, c:c + l] = i
            fill[r] = c + l
            cu.append(r * L + c)
        if fill[r] < L:
            cu.append(r * L + int(fill[r]))
    rows_w = min(len(p.rows), R)
    cu.append(rows_w * L)
    cu_out = np.full(n + R + 1, -1, dtype=np.int32)       # (entries behind n[2] are not written: -1 stands for "whatever was there")
    cu_out[:len(cu)] = cu
    nn = np.array([len(p.rows), sum(p.clen), len(cu), sum(1 for i in range(n) if p.cut[i] and p.clen[i])], dtype=np.int64)
    return Packed(ids, lab, byt, mask, pos, sid, p.place, fill, cu_out, nn, 1 if len(bad) else 0)


def check_invariants(out, lengths, row_len, max_rows):
    """what holds for every plan: each non-empty sequence once and contiguous, fills within the row, positions and boundaries agree with
    seq_place.  out: Packed (of the device, the simulator or pack())."""
    clen, _ = clip(lengths, row_len)
    rows = int(out.n[0])
    rows_w = min(rows, max_rows)
    assert (out.row_fill[:rows_w] <= row_len).all() and (out.row_fill[:rows_w] >= 1).all() and (out.row_fill[rows_w:] == 0).all()
    flat_sid, flat_pos = out.seq_ids.reshape(-1), out.position_ids.reshape(-1)
    starts = []
    for i, l in enumerate(clen):
        r, c = (int(x) for x in out.seq_place[i])
        if l == 0:
            assert (r, c) == (-1, -1)
            continue
        assert 0 <= r < rows and 0 <= c and c + l <= row_len
        where = np.nonzero(flat_sid == i)[0]
        if r >= rows_w:
            assert len(where) == 0
            continue
        e = r * row_len + c
        assert len(where) == l and where[0] == e and where[-1] == e + l - 1
        assert (flat_pos[e:e + l] == np.arange(l)).all()
        starts.append(e)
    assert int((flat_sid >= 0).sum()) == sum(l for i, l in enumerate(clen) if l and int(out.seq_place[i, 0]) < rows_w)
    for r in range(rows_w):
        if out.row_fill[r] < row_len:
            starts.append(r * row_len + int(out.row_fill[r]))
    starts.append(rows_w * row_len)
    k = int(out.n[2])
    assert k == len(starts) and (out.cu_seqlens[:k] == np.array(sorted(starts))).all()
    assert int(out.n[1]) == sum(clen)
