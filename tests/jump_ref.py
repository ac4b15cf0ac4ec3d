"""Jump-forward for the regex guide, the DEFINITION (include/splintr_hip.h, spl_dfa_jump_index_device / spl_dfa_jump_device): the forced
byte, the run, the UTF-8 trim and the jump step by brute force -- every byte of a row counted, every run walked from its state, nothing
tabulated.  walk, DEAD, ORDINARY, b(t) and the state are tests/dfa_ref.py's: a table is (trans, accept), a state (q, constrained, broken,
done), `toks` the list of the ordinary tokens."""
import numpy as np

import dfa_ref as ref
import heal_ref

MAX_BYTES = 64
MAX_IDS = 64
INDEX_BYTES_PER_STATE = 64 * 4 + 1 + 1 + 64


def index_bytes(n_states):
    return n_states * INDEX_BYTES_PER_STATE


def force(tab, q):
    """The byte state q forces, or None: q does not accept and exactly one byte leads to a state (a value >= S is DEAD)."""
    trans, accept = tab
    S = ref.n_states(tab)
    if accept[q]:
        return None
    live = [x for x in range(256) if int(trans[q][x]) < S]
    return live[0] if len(live) == 1 else None


def raw_run(tab, q, cap=MAX_BYTES):
    """The forced bytes from state q, capped, before the trim."""
    out = bytearray()
    while len(out) < cap:
        x = force(tab, q)
        if x is None:
            break
        out.append(x)
        q = int(tab[0][q][x])
    return bytes(out)


def need(lead):
    """The continuation bytes a lead byte (>= 0xC0) announces."""
    return 3 if lead >= 0xF0 else (2 if lead >= 0xE0 else 1)


def trim(data):
    """Cut back to a character boundary of the bytes themselves: continuation bytes are taken off the end until a lead byte shows; if it
    has fewer of them behind it than it announces, the run ends in front of it.  Leading continuation bytes stay."""
    k = len(data)
    while k > 0 and 0x80 <= data[k - 1] < 0xC0:
        k -= 1
    if k > 0 and data[k - 1] >= 0xC0 and len(data) - k < need(data[k - 1]):
        return bytes(data[:k - 1])
    return bytes(data)


def run(tab, q):
    return trim(raw_run(tab, q))


def runs(tab):
    return [run(tab, q) for q in range(ref.n_states(tab))]


def run_arrays(tab):
    """(run uint8 [S, 64], run_len uint8 [S]) as the jump index holds them: zeros behind a run."""
    S = ref.n_states(tab)
    arr = np.zeros((S, MAX_BYTES), dtype=np.uint8)
    lens = np.zeros(S, dtype=np.uint8)
    for q, r in enumerate(runs(tab)):
        arr[q, :len(r)] = np.frombuffer(r, dtype=np.uint8)
        lens[q] = len(r)
    return arr, lens


def jump(toks, tab, state, row, n_ids, row_len_out):
    """THE JUMP of a loaded, stepped state: (state behind what was emitted, the emitted ids).  row: the state's 64 ids of the jump index
    as they lie there, n_ids its count -- neither is trusted."""
    q, con, broken, done = state
    if not con:
        return state, []
    out = []
    for t in list(row)[:min(int(n_ids), MAX_IDS, row_len_out)]:
        b = heal_ref._bytes_of(toks, int(t))
        q1 = ref.walk(tab, q, b) if b is not None else ref.DEAD
        if q1 == ref.DEAD:
            break
        q = q1
        out.append(int(t))
    return (q, True, False, False), out


def call(toks, tab, state, ids, jump_ids, jump_n, row_len_out, n_words, end_ids=()):
    """What one jump call does to a state word as it lies in memory -> (state written back, mask row, emitted ids).  jump_ids [S, 64] and
    jump_n [S]: the jump index's ids and counts."""
    s = ref.step(toks, tab, ref.load(tab, state), ids, end_ids)
    emitted = []
    if s[1]:
        s, emitted = jump(toks, tab, s, jump_ids[s[0]], jump_n[s[0]], row_len_out)
    s = ref.settle(toks, tab, s, end_ids)
    return s, ref.mask(toks, tab, s, n_words, end_ids), emitted


def greedy_ids(toks, data):
    """Some ids whose bytes spell `data` (longest token first), or None: a stand-in for an encoder where a test needs ids that walk."""
    by_bytes = {}
    for i, b in toks:
        by_bytes.setdefault(bytes(b), i)
    out, at = [], 0
    while at < len(data):
        for n in range(len(data) - at, 0, -1):
            i = by_bytes.get(bytes(data[at:at + n]))
            if i is not None:
                out.append(i)
                at += n
                break
        else:
            return None
    return out


def pack_index(ids, n_ids, run_len=None, run=None):
    """A jump index as it lies in memory, uint8 [S * 322] on a 4-byte aligned base, from its parts (ids [S, 64], n_ids [S], ...)."""
    S = len(n_ids)
    buf = np.zeros(S * INDEX_BYTES_PER_STATE // 4 + 1, dtype=np.uint32).view(np.uint8)[:S * INDEX_BYTES_PER_STATE]
    buf[:256 * S] = np.ascontiguousarray(np.asarray(ids).astype(np.uint32)).reshape(S, MAX_IDS).view(np.uint8).reshape(-1)
    buf[256 * S:257 * S] = np.asarray(n_ids).astype(np.uint8)
    if run_len is not None:
        buf[257 * S:258 * S] = np.asarray(run_len, dtype=np.uint8)
    if run is not None:
        buf[258 * S:] = np.ascontiguousarray(run, dtype=np.uint8).reshape(-1)
    return buf


def index_parts(buf, n_states):
    """(ids uint32 [S, 64], n_ids uint8 [S], run_len uint8 [S], run uint8 [S, 64]) of a jump index's bytes."""
    S = n_states
    buf = np.asarray(buf, dtype=np.uint8)
    assert buf.size == index_bytes(S)
    return (np.frombuffer(buf[:256 * S].tobytes(), dtype=np.uint32).reshape(S, MAX_IDS), buf[256 * S:257 * S].copy(), buf[257 * S:258 * S].copy(),
            buf[258 * S:].reshape(S, MAX_BYTES).copy())


def index_of(toks, tab, encode=None):
    """The jump index of a table by the definition: the runs, and their ids by `encode(bytes) -> ids or None` (default: greedy_ids -- a
    stand-in, the product encodes with the tokenizer's own encoder)."""
    enc = encode if encode is not None else (lambda data: greedy_ids(toks, data))
    S = ref.n_states(tab)
    arr, lens = run_arrays(tab)
    ids = np.zeros((S, MAX_IDS), dtype=np.uint32)
    n_ids = np.zeros(S, dtype=np.uint8)
    for q in range(S):
        got = enc(bytes(arr[q, :lens[q]])) if lens[q] else []
        if got:
            ids[q, :len(got)] = got
            n_ids[q] = len(got)
    return pack_index(ids, n_ids, lens, arr)
