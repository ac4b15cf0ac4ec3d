"""What spl_pair_device must produce, restated with plain loops (TEST TOOL).

Written from the semantics in include/splintr_hip.h, not from the kernel: a row is built as a Python list -- prefix + A' + middle + B' +
suffix -- and padded.  LONGEST_FIRST is Hugging Face's SEQUENTIAL rule (one id at a time from the longer side, from B on a tie), not the
closed form the kernel evaluates.  Values are kept as uint64 holding the 32-bit pattern, so an int64 output must EQUAL them (zero
extension) and an int32 output must equal their low 32 bits.
"""
import numpy as np

I64, PAD_LEFT, KEEP_TAIL_A, KEEP_TAIL_B = 1, 2, 32, 64
LONGEST_FIRST, ONLY_FIRST, ONLY_SECOND = 0, 1, 2


def truncate(la, lb, budget, trunc):
    """-> (a', b'): the ids kept of each side"""
    a, b = la, lb
    if trunc == ONLY_SECOND:
        a = min(la, budget)
        b = min(lb, budget - a)
    elif trunc == ONLY_FIRST:
        b = min(lb, budget)
        a = min(la, budget - b)
    else:
        assert trunc == LONGEST_FIRST
        while a + b > budget:
            if a > b:
                a -= 1
            else:                      # the longer side; B on a tie
                b -= 1
    return a, b


def _doc(ids, off, n, i):
    """document i of a side as a list; (list, bad): an index outside 0 .. n - 1 names the empty document"""
    if i < 0 or i >= n:
        return [], True
    return [int(x) for x in ids[int(off[i]):int(off[i + 1])]], False


def pair_row(a, b, L, flags, trunc, prefix, middle, suffix):
    """the entries of one row that are not padding, as (value, type, special) triples, and (a', b')"""
    k = len(prefix) + len(middle) + len(suffix)
    na, nb = truncate(len(a), len(b), L - k, trunc)
    a = a[len(a) - na:] if flags & KEEP_TAIL_A else a[:na]
    b = b[len(b) - nb:] if flags & KEEP_TAIL_B else b[:nb]
    row = [(x, 0, 1) for x in prefix] + [(x, 0, 0) for x in a] + [(x, 0, 1) for x in middle] + \
          [(x, 1, 0) for x in b] + [(x, 1, 1) for x in suffix]
    return row, (na, nb)


def pair_ref(a_ids, a_off, n_a, b_ids, b_off, n_b, a_idx, b_idx, n_pairs, L, flags, pad_id, trunc=LONGEST_FIRST, prefix=(), middle=(),
             suffix=()):
    """-> rows uint64 [n_pairs, L], mask, type, special uint8 [n_pairs, L], lengths int32 [n_pairs], kept int32 [n_pairs, 2], status.
    a_off / b_off: at least n + 1 ABSOLUTE offsets into that side's ids (off[0] need not be 0); a_idx / b_idx: None for the identity."""
    k = len(prefix) + len(middle) + len(suffix)
    assert L > 0 and L >= k
    rows = np.full((n_pairs, L), pad_id, dtype=np.uint64)
    mask = np.zeros((n_pairs, L), dtype=np.uint8)
    ttype = np.zeros((n_pairs, L), dtype=np.uint8)
    special = np.ones((n_pairs, L), dtype=np.uint8)
    lens = np.zeros(n_pairs, dtype=np.int32)
    kept = np.zeros((n_pairs, 2), dtype=np.int32)
    status = 0
    for p in range(n_pairs):
        a, bad_a = _doc(a_ids, a_off, n_a, p if a_idx is None else int(a_idx[p]))
        b, bad_b = _doc(b_ids, b_off, n_b, p if b_idx is None else int(b_idx[p]))
        status |= 1 if bad_a or bad_b else 0
        row, kept[p] = pair_row(a, b, L, flags, trunc, list(prefix), list(middle), list(suffix))
        at = L - len(row) if flags & PAD_LEFT else 0
        for i, (x, t, s) in enumerate(row):
            rows[p, at + i], mask[p, at + i], ttype[p, at + i], special[p, at + i] = x, 1, t, s
        lens[p] = len(row)
    return rows, mask, ttype, special, lens, kept, status


def sweep_lengths(budget, n, rng):
    """document lengths drawn to hit 0, half the budget +- 1 and the budget +- 1 (negative ones count as 0), and one far beyond"""
    h = budget // 2
    pool = [max(0, x) for x in (0, 1, h - 1, h, h + 1, (budget + 1) // 2, budget - 1, budget, budget + 1, 2 * budget + 3)]
    return [pool[i] for i in rng.integers(0, len(pool), size=n)]


def csr(doc_lens, rng, base=0):
    """ids uint32 (random bit patterns, among them 0xFFFFFFFF, 0x80000001 and 0xFFFFFFFD) and ABSOLUTE offsets uint64 that start at
    `base`: the ids array holds `base` entries of filler in front"""
    off = np.full(len(doc_lens) + 1, base, dtype=np.uint64)
    if len(doc_lens):
        off[1:] += np.cumsum(np.asarray(doc_lens, dtype=np.uint64))
    T = int(off[-1])
    ids = rng.integers(0, 1 << 32, size=T, dtype=np.uint64).astype(np.uint32)
    edge = np.array([0xFFFFFFFF, 0x80000001, 0xFFFFFFFD, 0, 0x7FFFFFFF, 0x80000000], dtype=np.uint32)
    m = min(T - base, len(edge))
    ids[base:base + m] = edge[:m]
    if T - base > 12:
        ids[-6:] = edge
    return ids, off


# ------------------------------------------------------------------------------------------ the grid both test files run
N_A, N_B = 9, 11                       # documents of the two sides of a grid case
ROW_LENS = list(range(1, 10)) + [63, 64, 65]
LONG_ROW_LENS = [96, 99, 130]          # rows that hold three full fixed segments (3 * 32 ids)
KINDS = ["identity", "reversed", "same", "one_side", "bad"]
FLAG_SETS = (0, PAD_LEFT, KEEP_TAIL_A, KEEP_TAIL_B, KEEP_TAIL_A | KEEP_TAIL_B, PAD_LEFT | KEEP_TAIL_A, PAD_LEFT | KEEP_TAIL_B,
             PAD_LEFT | KEEP_TAIL_A | KEEP_TAIL_B)


def segments(L):
    """the fixed segments tried at row length L -- counts (0,0,0), (1,1,1), (1,2,1), (32,32,32) and one with k == L, those that fit --
    as (prefix, middle, suffix) with values that tell the segments apart"""
    counts = [(0, 0, 0), (1, 1, 1), (1, 2, 1), (32, 32, 32)]
    counts.append((L, 0, 0) if L <= 32 else (32, min(32, L - 32), L - 32 - min(32, L - 32)))        # k == row_len
    out = []
    for c in counts:
        if sum(c) <= L and max(c) <= 32 and c not in [tuple(map(len, x)) for x in out]:
            out.append((tuple(0xA0000000 + i for i in range(c[0])), tuple(0xB0000000 + i for i in range(c[1])),
                        tuple(0xC0000000 + i for i in range(c[2]))))
    return out


def indices(kind, n_pairs, rng):
    """-> (a_idx, b_idx, whether an index among them names no document)"""
    if kind == "identity":
        return None, None, False
    if kind == "reversed":
        return [N_A - 1 - p for p in range(n_pairs)], [N_B - 1 - p for p in range(n_pairs)], False
    if kind == "same":
        return [3] * n_pairs, [0] * n_pairs, False
    if kind == "one_side":
        return None, [int(x) for x in rng.integers(0, N_B, size=n_pairs)], False
    assert kind == "bad"
    a, b = [int(x) for x in rng.integers(0, N_A, size=n_pairs)], [int(x) for x in rng.integers(0, N_B, size=n_pairs)]
    a[0], b[-1] = -1, N_B
    a[n_pairs // 2] = N_A
    return a, b, True


def grid(L, seed):
    """The cases of one row length: every fixed-segment set that fits x every truncation mode x both tail flags x both padding sides,
    with document lengths drawn around 0, half the budget and the budget; per combination one CSR pair and, on it, every kind of index
    array with n_pairs running through 5 .. 8 (so that n_pairs * L % 4 takes every value L allows).
    Yields (src = (a_ids, a_off, N_A, b_ids, b_off, N_B), [(kind, a_idx, b_idx, bad, n_pairs), ...], L, flags, trunc, segs)."""
    rng = np.random.default_rng(seed)
    count = 0
    for segs in segments(L):
        k = sum(map(len, segs))
        if L in LONG_ROW_LENS and k != 96:
            continue
        for trunc in (LONGEST_FIRST, ONLY_FIRST, ONLY_SECOND):
            for flags in FLAG_SETS:
                a_ids, a_off = csr(sweep_lengths(L - k, N_A, rng), rng)
                b_ids, b_off = csr(sweep_lengths(L - k, N_B, rng), rng)
                calls = []
                for kind in KINDS:
                    n_pairs = 5 + count % 4
                    calls.append((kind,) + indices(kind, n_pairs, rng) + (n_pairs,))
                    count += 1
                yield (a_ids, a_off, N_A, b_ids, b_off, N_B), calls, L, flags, trunc, segs
