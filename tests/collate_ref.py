"""What spl_pad_device / spl_pack_device must produce, restated with plain loops over numpy arrays (TEST TOOL).

Written from the semantics in include/splintr_hip.h, not from the kernels: the padded rows are built document by document, the packed
stream by appending [BOS] ids [EOS] per document and cutting the result into rows.  Values are kept as uint64 holding the 32-bit
pattern, so an int64 output must EQUAL them (zero extension) and an int32 output must equal their low 32 bits.
"""
import numpy as np

I64, PAD_LEFT, KEEP_TAIL, BOS, EOS = 1, 2, 4, 8, 16


def n_special(flags):
    return (1 if flags & BOS else 0) + (1 if flags & EOS else 0)


def pad_ref(ids, off, L, flags, pad_id, bos_id=0, eos_id=0):
    """-> rows uint64 [n_docs, L], mask uint8 [n_docs, L], lengths int32 [n_docs]"""
    n_docs = len(off) - 1
    k = n_special(flags)
    assert L >= k and L > 0
    rows = np.full((n_docs, L), pad_id, dtype=np.uint64)
    mask = np.zeros((n_docs, L), dtype=np.uint8)
    lens = np.zeros(n_docs, dtype=np.int32)
    for d in range(n_docs):
        toks = [int(x) for x in ids[int(off[d]):int(off[d + 1])]]
        budget = L - k
        if len(toks) > budget:
            toks = toks[len(toks) - budget:] if flags & KEEP_TAIL else toks[:budget]
        row = ([bos_id] if flags & BOS else []) + toks + ([eos_id] if flags & EOS else [])
        at = L - len(row) if flags & PAD_LEFT else 0
        for i, x in enumerate(row):
            rows[d, at + i] = x
            mask[d, at + i] = 1
        lens[d] = len(row)
    return rows, mask, lens


def pack_ref(ids, off, L, flags, pad_id, bos_id=0, eos_id=0):
    """-> rows uint64 [n_rows, L], doc int32 [n_rows, L], pos int32 [n_rows, L], n_rows, S"""
    n_docs = len(off) - 1
    assert L > 0 and not flags & (PAD_LEFT | KEEP_TAIL)
    stream, doc, start = [], [], []
    for d in range(n_docs):
        piece = ([bos_id] if flags & BOS else []) + [int(x) for x in ids[int(off[d]):int(off[d + 1])]] + ([eos_id] if flags & EOS else [])
        doc_start = len(stream)
        for x in piece:
            stream.append(x)
            doc.append(d)
            start.append(doc_start)
    S = len(stream)
    n_rows = (S + L - 1) // L
    rows = np.full(n_rows * L, pad_id, dtype=np.uint64)
    docs = np.full(n_rows * L, -1, dtype=np.int32)
    pos = np.zeros(n_rows * L, dtype=np.int32)
    for p in range(S):
        rows[p] = stream[p]
        docs[p] = doc[p]
        pos[p] = p - max(start[p], (p // L) * L)       # restarts at a document's start and at a row's start
    return rows.reshape(n_rows, L), docs.reshape(n_rows, L), pos.reshape(n_rows, L), n_rows, S


def csr(doc_lens, rng=None, edge_ids=True):
    """ids uint32 (random bit patterns; the first few are the edge values 0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE) and offsets uint64"""
    off = np.zeros(len(doc_lens) + 1, dtype=np.uint64)
    if len(doc_lens):
        off[1:] = np.cumsum(np.asarray(doc_lens, dtype=np.uint64))
    T = int(off[-1])
    rng = rng or np.random.default_rng(1)
    ids = rng.integers(0, 1 << 32, size=T, dtype=np.uint64).astype(np.uint32)
    if edge_ids:
        edge = np.array([0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE], dtype=np.uint32)
        ids[:min(T, 4)] = edge[:min(T, 4)]
        if T > 8:
            ids[-4:] = edge
    return ids, off


def sweep_lengths(L, k, n_docs, rng):
    """document lengths drawn from {0, 1, L-k-1, L-k, L-k+1, 2L+3} (negative ones count as 0)"""
    pool = [max(0, x) for x in (0, 1, L - k - 1, L - k, L - k + 1, 2 * L + 3)]
    return [pool[i] for i in rng.integers(0, len(pool), size=n_docs)]
