"""N-gram drafting, restated: the definition of spl_ngram_draft_device (include/splintr_hip.h) in plain Python, brute force.  Lists of
Python ints in, lists out; nothing is shared with the library."""


def hole(v):
    return not 0 <= v < (1 << 31)


def ngram_ref(hist, length, new, new_len, cap, *, min_n, max_n, depth, branches=1, earliest=False, pad_id=0):
    """One sequence: hist (cap values), new (a row, may be empty) -> dict(hist, length, full, ids, count, match, from_, parent); the draft
    fields are None for depth 0."""
    length = min(max(length, 0), cap)
    new_len = min(max(new_len, 0), len(new))
    H = (list(hist[:length]) + list(new[:new_len]))[:cap]
    L = len(H)
    out = dict(hist=H + list(hist[L:]), length=L, full=int(length + new_len > cap), ids=None, count=None, match=None, from_=None, parent=None)
    if not depth:
        return out
    cands = []
    for e in range(1, L):
        m = 0
        for n in range(1, min(max_n, e) + 1):
            if all(not hole(H[e - k]) and H[e - k] == H[L - k] for k in range(1, n + 1)):
                m = n
        if m >= min_n and not hole(H[e]):
            cands.append((m, e))
    cands.sort(key=lambda c: (-c[0], c[1] if earliest else -c[1]))
    ids, parent = [pad_id] * (branches * depth), [-2] * (branches * depth)
    count, match, from_, firsts = [0] * branches, [0] * branches, [-1] * branches, []
    for m, e in cands:
        j = len(firsts)
        if j == branches:
            break
        if H[e] in firsts:
            continue
        firsts.append(H[e])
        run = H[e:min(e + depth, L)]
        holes = [k for k, v in enumerate(run) if hole(v)]
        run = run[:holes[0]] if holes else run
        for k, v in enumerate(run):
            ids[j * depth + k], parent[j * depth + k] = v, (j * depth + k - 1 if k else -1)
        count[j], match[j], from_[j] = len(run), m, e
    out.update(ids=ids, count=count, match=match, from_=from_, parent=parent)
    return out
