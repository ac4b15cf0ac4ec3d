"""What spl_chat_device must produce, restated with plain loops (TEST TOOL).

Written from the semantics in include/splintr_hip.h, not from the kernels: the body of a conversation is built as a Python list of
entries -- header + content + footer per turn --, whole leading turns are removed by trying t0 = 0, 1, ... in turn, the list is cut and
the row padded.  Values are kept as uint64 holding the 32-bit pattern, so an int64 row must EQUAL them (zero extension) and an int32 row
must equal their low 32 bits; labels are int64 NUMBERS: a trained entry's id zero-extended, ignore_id sign-extended from 32 bits.
"""
from collections import namedtuple

import numpy as np

from pair_ref import csr

I64, PAD_LEFT, DROP_OLDEST, PIN_FIRST = 1, 2, 32, 64
NO_ROLE = 255
MAX_ROLES, MAX_HEADER, MAX_FOOTER, MAX_BOS, MAX_GEN = 8, 16, 8, 8, 16
PAD_ID, IGNORE_ID = 0xFFFFFFFF, 0xFFFFFF9C            # (-100 as 32 bits)
UNWRITTEN = -7                                         # d_turn_col of a turn that no valid conversation contains

Template = namedtuple("Template", "roles bos gen train_content train_footer")          # roles: [(header ids, footer ids)] by role number
Out = namedtuple("Out", "rows labels loss mask role special lens kept turn_col status")
Entry = namedtuple("Entry", "value role special trained")


def _signed32(x):
    return x - (1 << 32) if x & 0x80000000 else x


def turn_entries(ids, off, n_docs, doc, role, trainable, tpl):
    """-> (entries of header + content + footer, entries in the header, entries of content, bad)"""
    if role >= len(tpl.roles):
        return [], 0, 0, True                                       # contributes nothing
    header, footer = tpl.roles[role]
    bad = doc < 0 or doc >= n_docs
    content = [] if bad else [int(x) for x in ids[int(off[doc]):int(off[doc + 1])]]
    tc = bool((tpl.train_content >> role) & 1) and trainable
    tf = tc and bool((tpl.train_footer >> role) & 1)
    ent = [Entry(x, role, 1, False) for x in header] + [Entry(x, role, 0, tc) for x in content] + [Entry(x, role, 1, tf) for x in footer]
    return ent, len(header), len(content), bad


def chat_ref(ids, off, n_docs, turn_doc, turn_role, turn_train, n_turns, conv_off, n_convs, L, flags, tpl, pad_id=PAD_ID,
             ignore_id=IGNORE_ID, where=None):
    """-> Out.  where (a list, optional) receives per conversation with a cut on the right what the first entry cut away was:
    "header", "content", "footer" together with whether it was the FIRST entry of that part (the cut is exactly at a seam)."""
    n_bos, n_gen = len(tpl.bos), len(tpl.gen)
    B = L - n_bos - n_gen
    assert L > 0 and B >= 0
    assert not (flags & PIN_FIRST) or (flags & DROP_OLDEST)
    rows = np.full((n_convs, L), pad_id, dtype=np.uint64)
    labels = np.full((n_convs, L), _signed32(ignore_id), dtype=np.int64)
    loss = np.zeros((n_convs, L), dtype=np.uint8)
    mask = np.zeros((n_convs, L), dtype=np.uint8)
    role = np.full((n_convs, L), NO_ROLE, dtype=np.uint8)
    special = np.ones((n_convs, L), dtype=np.uint8)
    lens = np.zeros(n_convs, dtype=np.int32)
    kept = np.zeros((n_convs, 2), dtype=np.int32)
    turn_col = np.full((n_turns, 2), UNWRITTEN, dtype=np.int32)
    status = 0
    for c in range(n_convs):
        a, b = int(conv_off[c]), int(conv_off[c + 1])
        if b < a or b > n_turns:
            status = 1
            a = b = 0
        turns = []
        for t in range(a, b):
            doc = t if turn_doc is None else int(turn_doc[t])
            ent, nh, nc, bad = turn_entries(ids, off, n_docs, doc, int(turn_role[t]), True if turn_train is None else bool(turn_train[t]), tpl)
            status |= 1 if bad else 0
            turns.append((t, ent, nh, nc, bad))
        n = len(turns)
        keep = list(range(n))
        if flags & DROP_OLDEST and n:
            pinned = bool(flags & PIN_FIRST) and n >= 2
            head = [0] if pinned else []
            keep = head + [n - 1]                                   # if no t0 fits: the last turn alone (after turn 0 when pinned)
            for t0 in range(1 if pinned else 0, n):
                if sum(len(turns[i][1]) for i in head) + sum(len(turns[i][1]) for i in range(t0, n)) <= B:
                    keep = head + list(range(t0, n))
                    break
        body, content_at = [], {}
        for i in keep:
            t, ent, nh, nc, bad = turns[i]
            content_at[i] = len(body) + nh
            body += [(e, i, "header" if j < nh else "content" if j < nh + nc else "footer", j in (0, nh, nh + nc)) for j, e in enumerate(ent)]
        cut = max(0, len(body) - B)
        if cut and where is not None:
            where.append(body[B][2:])
        body = body[:B]
        row = [Entry(x, NO_ROLE, 1, False) for x in tpl.bos] + [x[0] for x in body] + [Entry(x, NO_ROLE, 1, False) for x in tpl.gen]
        at = L - len(row) if flags & PAD_LEFT else 0
        for i, e in enumerate(row):
            rows[c, at + i], mask[c, at + i], role[c, at + i], special[c, at + i] = e.value, 1, e.role, e.special
            if e.trained:
                labels[c, at + i], loss[c, at + i] = e.value, 1
        lens[c] = len(row)
        kept[c] = (n - len(keep), min(cut, (1 << 31) - 1))
        for i, (t, ent, nh, nc, bad) in enumerate(turns):
            turn_col[t] = (-1, -1)
            if i in content_at and not bad and content_at[i] < len(body):
                turn_col[t] = (at + n_bos + content_at[i], at + n_bos + min(content_at[i] + nc, len(body)))
    return Out(rows, labels, loss, mask, role, special, lens, kept, turn_col, status)


# ------------------------------------------------------------------------------------------ the grid both test files run
ROW_LENS = [1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 130]
TURN_COUNTS = [0, 1, 2, 63, 64, 65, 130]
FLAG_SETS = (0, PAD_LEFT, DROP_OLDEST, DROP_OLDEST | PAD_LEFT, DROP_OLDEST | PIN_FIRST, DROP_OLDEST | PIN_FIRST | PAD_LEFT)
Case = namedtuple("Case", "ids off n_docs turn_doc turn_role turn_train n_turns conv_off n_convs L flags tpl")


def templates(L):
    """the three templates tried at row length L: one role without any template entry; three roles with mixed counts; eight roles with
    every count at its maximum where the row holds bos + gen (otherwise as many of them as fit).  Values tell the parts apart."""
    def ids(base, n):
        return tuple(base + j for j in range(n))

    def fit(n_bos, n_gen):                              # bos first, then gen, cut to the row
        n_bos = min(n_bos, L)
        return n_bos, min(n_gen, L - n_bos)
    out = [Template([((), ())], (), (), 1, 1)]
    nb, ng = fit(1, 3)
    out.append(Template([(ids(0xA0000000, 2), ids(0xB0000000, 1)), (ids(0xA0000100, 0), ids(0xB0000100, 2)), (ids(0xA0000200, 3), ids(0xB0000200, 0))],
                        ids(0xC0000000, nb), ids(0xD0000000, ng), 0b100, 0b100))
    nb, ng = fit(MAX_BOS, MAX_GEN)
    counts = [(MAX_HEADER, MAX_FOOTER), (0, 0), (MAX_HEADER, 0), (0, MAX_FOOTER), (1, 1), (5, 3), (MAX_HEADER, MAX_FOOTER), (2, 0)]
    out.append(Template([(ids(0xA0000000 + 256 * r, h), ids(0xB0000000 + 256 * r, f)) for r, (h, f) in enumerate(counts)],
                        ids(0xC0000000, nb), ids(0xD0000000, ng), 0b01010101, 0b01000100))
    return out


def build(convs, L, flags, tpl, rng, identity, train, base=0):
    """convs: a list of conversations, each a list of (role, content length) -> Case.  identity: turn_doc is None and the documents lie in
    turn order; otherwise they are shuffled and turns with equally long contents may share one.  train: turn_train is given (random bytes)."""
    want = [ln for conv in convs for _, ln in conv]
    n_turns = len(want)
    if identity:
        doc_lens, turn_doc = want, None
    else:
        doc_lens, by_len, turn_doc = [], {}, []
        for ln in want:
            if ln in by_len and rng.integers(0, 3) == 0:
                turn_doc.append(by_len[ln])
            else:
                by_len[ln] = len(doc_lens)
                turn_doc.append(len(doc_lens))
                doc_lens.append(ln)
        perm = rng.permutation(len(doc_lens))           # document perm[i] of the CSR is document i of the list
        inv = np.argsort(perm)
        doc_lens = [doc_lens[int(i)] for i in perm]
        turn_doc = np.array([int(inv[d]) for d in turn_doc], dtype=np.int32)
    ids, off = csr(doc_lens, rng, base)
    turn_role = np.array([r for conv in convs for r, _ in conv], dtype=np.uint8)
    turn_train = rng.integers(0, 3, size=n_turns).astype(np.uint8) * 127 if train else None
    conv_off = np.zeros(len(convs) + 1, dtype=np.uint64)
    conv_off[1:] = np.cumsum([len(conv) for conv in convs])
    return Case(ids, off, len(doc_lens), turn_doc, turn_role, turn_train, n_turns, conv_off, len(convs), L, flags, tpl)


def conversations(L, tpl, rng):
    """The conversations of one grid case.  (1) every turn count of TURN_COUNTS with short random contents; (2) two-turn conversations
    whose first content is as long as it takes for the budget to end x entries into the SECOND turn, x running over every entry of its
    header, content and footer and one beyond (cuts inside each part and exactly at each seam); (3) for DROP_OLDEST: a last turn that
    alone exceeds the budget (nothing fits), two long turns in front of a short one (only the last fits), a first turn that alone
    exceeds the budget (the pinned turn fills the row)."""
    n_roles = len(tpl.roles)
    B = L - len(tpl.bos) - len(tpl.gen)
    role = lambda: int(rng.integers(0, n_roles))
    ext = lambda r, ln: len(tpl.roles[r][0]) + ln + len(tpl.roles[r][1])
    convs = [[(role(), int(rng.integers(0, 4))) for _ in range(n)] for n in TURN_COUNTS]
    for r2 in range(n_roles):
        r1, len2 = (r2 + 1) % n_roles, 3
        for x in range(ext(r2, len2) + 2):
            len1 = B - x - ext(r1, 0)
            if len1 >= 0:
                convs.append([(r1, len1), (r2, len2)])
    convs.append([(role(), 1), (role(), 2), (role(), B + 5)])
    convs.append([(role(), B), (role(), B + 1), (role(), max(0, B - 24))])
    convs.append([(role(), B + 3), (role(), 1), (role(), 0)])
    convs.append([(role(), 2)])
    order = rng.permutation(len(convs))
    return [convs[int(i)] for i in order]


def grid(L, seed):
    """the cases of one row length: every template of templates(L) x every flag set; identity / shuffled documents, turn_train given or
    not and the offsets' base alternate"""
    rng = np.random.default_rng(seed)
    count = 0
    for tpl in templates(L):
        for flags in FLAG_SETS:
            yield build(conversations(L, tpl, rng), L, flags, tpl, rng, identity=count % 2 == 0, train=count % 3 == 1, base=5 * (count % 4 == 3))
            count += 1


BAD_KINDS = ["role", "doc_negative", "doc_beyond", "range_reversed", "range_beyond"]


def spoil(case, kind):
    """case with ONE bad input of the given kind; the arrays are copies"""
    turn_doc = np.arange(case.n_turns, dtype=np.int32) if case.turn_doc is None else case.turn_doc.copy()
    turn_role, conv_off = case.turn_role.copy(), case.conv_off.copy()
    c = next(c for c in range(case.n_convs) if conv_off[c + 1] - conv_off[c] >= 2)
    t = int(conv_off[c]) + 1
    if kind == "role":
        turn_role[t] = len(case.tpl.roles)
    elif kind == "doc_negative":
        turn_doc[t] = -1
    elif kind == "doc_beyond":
        turn_doc[t] = case.n_docs
    elif kind == "range_reversed":                      # the last conversation's end lies in front of its start (no other range moves)
        conv_off[-1] = conv_off[-2] - 1
    else:
        assert kind == "range_beyond"
        conv_off[-1] = case.n_turns + 1
    return case._replace(turn_doc=turn_doc, turn_role=turn_role, conv_off=conv_off)
