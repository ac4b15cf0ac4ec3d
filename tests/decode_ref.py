"""Pure-Python statement of spl_decode_batch_device's contract (include/splintr_hip.h), for the tests: per document the bytes of its
valid ids one after the other, the offsets, the clamping of a CSR to n_ids_cap and the cut at bytes_capacity.  Slow and obvious."""
import numpy as np

I64, PAD_LEFT, SKIP_SPECIAL = 1, 2, 4
POISON = 0xA5


class Table:
    """id -> bytes (vocabulary ids and special-only ids alike) plus the set of ids that ONLY the special map holds."""

    def __init__(self, tokens, special_only=()):
        self.tokens = {int(k): bytes(v) for k, v in tokens.items()}
        self.special_only = {int(i) for i in special_only}
        assert self.special_only <= set(self.tokens)

    def span(self, v, flags):
        """what ONE id value (a Python int: an int64 value may be negative or beyond 32 bits) decodes to"""
        v = int(v)
        if not flags & I64:
            v &= 0xFFFFFFFF                       # 32-bit input is a bit pattern
        if not 0 <= v < (1 << 32):
            return b""
        if flags & SKIP_SPECIAL and v in self.special_only:
            return b""
        return self.tokens.get(v, b"")


def _finish(docs, capacity):
    """per-document byte strings -> (bytes below the capacity, offsets [n_docs + 1], need)"""
    off = np.zeros(len(docs) + 1, dtype=np.uint64)
    if docs:
        off[1:] = np.cumsum([len(d) for d in docs])
    raw = b"".join(docs)
    need = len(raw)
    return raw[:need if capacity is None else min(need, capacity)], off, need


def decode_csr(tab, ids, ids_off, n_ids_cap, flags=0, capacity=None):
    """CSR mode: document d is ids[off[d] .. off[d + 1]) with every offset clamped to n_ids_cap; ids beyond the clamped end are never
    looked at (the caller may leave anything there)."""
    assert not flags & PAD_LEFT
    off = [min(int(x), int(n_ids_cap)) for x in ids_off]
    docs = [b"".join(tab.span(ids[i], flags) for i in range(off[d], off[d + 1])) for d in range(len(off) - 1)]
    return _finish(docs, capacity)


def decode_rows(tab, rows, lengths=None, flags=0, capacity=None):
    """rows mode: document r is row r; with lengths its first (PAD_LEFT: last) clamp(lengths[r], 0, row_len) entries"""
    rows = np.asarray(rows)
    n, L = rows.shape
    docs = []
    for r in range(n):
        k = L if lengths is None else max(0, min(int(lengths[r]), L))
        cols = range(L - k, L) if flags & PAD_LEFT else range(k)
        docs.append(b"".join(tab.span(rows[r, c], flags) for c in cols))
    return _finish(docs, capacity)


# the synthetic table of the CPU tests: lengths 0, 1, 2, 3, 4, 5, 15, 16, 17, 255 and 300; ids 20 .. 24 are special-only; a far
# special (beyond the dense range); every byte string distinct in every byte position that matters (byte j of id i = f(i, j))
SYN_LENGTHS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 255, 300]
SYN_MAX_ID = 31
SYN_FAR = (100300, 5_000_000, (1 << 31) - 1)


def synthetic_table():
    toks = {}
    for i, n in enumerate(SYN_LENGTHS):
        toks[i] = bytes((37 * i + 11 * j + 1) % 251 for j in range(n))
    for i in range(20, 25):
        toks[i] = bytes((i + 3 * j) % 256 for j in range(i - 17))          # specials in the dense range: 3 .. 7 bytes
    for k, i in enumerate(SYN_FAR):
        toks[i] = b"<|far%d|>" % k
    return Table(toks, special_only=set(range(20, 25)) | set(SYN_FAR))


def random_ids(rng, n, p_unknown=0.25):
    """n ids of the synthetic table: known ones of every length, unknown ones (holes, beyond the dense range), specials"""
    known = list(range(len(SYN_LENGTHS))) + list(range(20, 25)) + list(SYN_FAR)
    unknown = [12, 19, 25, 31, 32, 77, 100299, 100301, 0xFFFFFFFF]
    out = np.empty(n, dtype=np.uint32)
    for i in range(n):
        pool = unknown if rng.random() < p_unknown else known
        out[i] = pool[int(rng.integers(len(pool)))]
    return out
