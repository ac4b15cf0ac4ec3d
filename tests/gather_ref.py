"""The wire format of the ragged all-gather and what its unpack must leave, in numpy -- written from the comments of
include/splintr_hip.h ("Ragged all-gather", spl_gatherv_unpack_at), not from the kernels, and importing nothing of the product.

A slab is `cap_words` u32 words:  [0] T   [1] N   [2 .. 2 + N] the N + 1 local offsets (room for max_docs + 1)   ids from word 3 + max_docs.
Ids are u32 each, or -- "slab_pack24" -- three bytes each, little endian, back to back; that form keeps one word of slack at the end
of the id area (the unpacker reads whole words).  A RANK here is (ids, off): ids np.uint32[..], off np.uint64[N + 1] with off[0] == 0;
off[-1] is the T the rank CLAIMS (more than len(ids) only where a test describes a slab that overflowed).
"""
import numpy as np

FILL_WORD = 0xC3C3C3C3          # what build_slab leaves in every word (and byte) nothing was written to: a reader of padding shows


def ids_at(max_docs):
    return 3 + max_docs


def id_cap(cap_words, max_docs, p24):
    """ids one slab can carry"""
    area = cap_words - ids_at(max_docs)
    return ((area - 1) * 4) // 3 if p24 else area


def slab_words(max_tokens, max_docs, p24):
    """words of a slab made for max_tokens ids and max_docs documents (what the gatherers allocate per rank)"""
    return ((3 * max_tokens + 3) // 4 + 1 if p24 else max_tokens) + max_docs + 4


def build_slab(ids_u32, off, cap_words, max_docs, p24):
    ids = np.asarray(ids_u32, dtype=np.uint32)
    off = np.asarray(off, dtype=np.uint64)
    n = len(off) - 1
    assert n >= 0 and n <= max_docs and int(off[0]) == 0 and cap_words >= max_docs + 4
    assert int(off[-1]) < 1 << 32 and len(ids) <= int(off[-1])
    slab = np.full(cap_words, FILL_WORD, dtype=np.uint32)
    slab[0], slab[1] = int(off[-1]), n
    slab[2:2 + n + 1] = off.astype(np.uint32)
    at = ids_at(max_docs)
    k = min(len(ids), id_cap(cap_words, max_docs, p24))
    if not p24:
        slab[at:at + k] = ids[:k]
        return slab
    assert k == 0 or int(ids[:k].max()) < 1 << 24
    area = slab[at:].view(np.uint8)
    b = np.empty((k, 3), dtype=np.uint8)
    b[:, 0], b[:, 1], b[:, 2] = ids[:k] & 0xFF, (ids[:k] >> 8) & 0xFF, (ids[:k] >> 16) & 0xFF
    area[:3 * k] = b.reshape(-1)
    return slab


def parse_slab(slab, max_docs, p24):
    """(ids, off) of a slab: the inverse of build_slab (the ids the slab really holds: min(T, id_cap) of them)"""
    slab = np.asarray(slab, dtype=np.uint32)
    t, n = int(slab[0]), int(slab[1])
    off = slab[2:2 + n + 1].astype(np.uint64)
    at = ids_at(max_docs)
    k = min(t, id_cap(len(slab), max_docs, p24))
    if not p24:
        return slab[at:at + k].copy(), off
    b = slab[at:].view(np.uint8)[:3 * k].reshape(k, 3).astype(np.uint32)
    return b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16), off


def ref_unpack(ranks):
    """The global CSR of `ranks` in rank order: ids concatenated, every rank's offsets moved by the tokens of the ranks before it, one
    closing entry.  Returns (ids np.uint32[T_total], off np.uint64[N_total + 1])."""
    ids, off, tb = [np.zeros(0, np.uint32)], [], 0
    for r_ids, r_off in ranks:
        r_off = np.asarray(r_off, dtype=np.uint64)
        assert len(r_ids) == int(r_off[-1])
        ids.append(np.asarray(r_ids, dtype=np.uint32))
        off.append(r_off[:-1] + np.uint64(tb))
        tb += int(r_off[-1])
    off.append(np.array([tb], dtype=np.uint64))
    return np.concatenate(ids), np.concatenate(off)


def ref_unpack_waves(waves_of_ranks, all_ids_cap, all_off_cap, id_cap=None):
    """spl_gatherv_unpack_at called once per wave on ONE d_run that starts at {0, 0}.  Returns (ids np.uint32[all_ids_cap],
    off np.uint64[all_off_cap], run [tokens, documents], status, written_ids_mask, written_off_mask): positions at or beyond a capacity
    are not written (the masks say which were), status is 1 if any rank has T > id_cap (`id_cap`: of the slabs; None = never), tbase + T >
    all_ids_cap or dbase + N + 1 > all_off_cap, and run advances by what the slabs CLAIM."""
    ids, off = np.zeros(all_ids_cap, np.uint32), np.zeros(all_off_cap, np.uint64)
    m_ids, m_off = np.zeros(all_ids_cap, bool), np.zeros(all_off_cap, bool)
    run, status = [0, 0], 0
    for ranks in waves_of_ranks:
        tb, db = run
        for r, (r_ids, r_off) in enumerate(ranks):
            r_off = np.asarray(r_off, dtype=np.uint64)
            t, n = int(r_off[-1]), len(r_off) - 1
            if (id_cap is not None and t > id_cap) or tb + t > all_ids_cap or db + n + 1 > all_off_cap:
                status = 1
            nw = max(0, min(n + (1 if r == len(ranks) - 1 else 0), all_off_cap - db))      # (the last rank of a wave writes the closing entry)
            off[db:db + nw] = r_off[:nw] + np.uint64(tb)
            m_off[db:db + nw] = True
            k = max(0, min(t, len(r_ids), id_cap if id_cap is not None else t, all_ids_cap - tb))
            ids[tb:tb + k] = np.asarray(r_ids, dtype=np.uint32)[:k]
            m_ids[tb:tb + k] = True
            tb, db = tb + t, db + n
        run = [tb, db]
    return ids, off, run, status, m_ids, m_off
