"""spl_chat_device without a GPU: the C ABI's symbols, struct layout and refusals, the mapping code the kernels run (splintr_amd/csrc/
spl_k_chat.h, evaluated for every output element by tests/hostsim/chat_sim.cpp, which also restates k_chat_turns' wavefront walk) against
tests/chat_ref.py, chat_ref against examples written out by hand, and the built-in templates against the CPU oracle's encode of the
rendered string."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import chat_ref as ref
from chat_ref import DROP_OLDEST, I64, IGNORE_ID, PAD_ID, PAD_LEFT, PIN_FIRST, Template
from conftest import ROOT

SPL_EINVAL = -1
OUTPUTS = ("labels", "loss", "mask", "role", "special", "len", "kept", "turn_col")


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as entry
    entry.build()
    from splintr_amd import _ffi
    return _ffi


@pytest.fixture(scope="module")
def sim():
    import chat_sim
    chat_sim.lib()
    return chat_sim


# ------------------------------------------------------------------------------------------ 1. the C ABI
def test_symbols_and_struct_layout(ffi):
    L = ffi.lib()
    for s in ("spl_chat_device", "spl_chat_work_bytes"):
        assert hasattr(L, s) and s in ffi.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "splintr_hip.h")).read()
    body = re.search(r"typedef struct spl_chat_opts \{(.*?)\} spl_chat_opts;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip() for decl in re.findall(r"uint32_t ([^;]+);", body) for n in decl.split(",")]
    assert fields == ["struct_size", "flags", "row_len", "pad_id", "ignore_id", "n_roles", "train_content", "train_footer", "n_bos", "n_gen",
                      "n_header[8]", "n_footer[8]", "bos[8]", "gen[16]", "header[8][16]", "footer[8][8]"]
    O = ffi.SplChatOpts
    names = [f[0] for f in O._fields_]
    assert names == [f.split("[")[0] for f in fields]
    assert ctypes.sizeof(O) == 968
    assert [getattr(O, n).offset for n in names] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 72, 104, 136, 200, 712]
    o = O(3, 50, 7, -100, [((1, 2), (3,)), ((), (4, 5))], 2, 2, bos=(9,), gen=(8, 8, 8))
    assert (o.struct_size, o.flags, o.row_len, o.pad_id, o.ignore_id, o.n_roles, o.train_content, o.train_footer, o.n_bos, o.n_gen) == \
        (968, 3, 50, 7, 0xFFFFFF9C, 2, 2, 2, 1, 3)
    assert list(o.n_header[:3]) == [2, 0, 0] and list(o.n_footer[:3]) == [1, 2, 0]
    assert list(o.header[0][:2]) == [1, 2] and o.footer[0][0] == 3 and list(o.footer[1][:2]) == [4, 5] and o.bos[0] == 9 and list(o.gen[:3]) == [8, 8, 8]
    for name, val in (("DROP_OLDEST", 32), ("PIN_FIRST", 64), ("NO_ROLE", 255), ("MAX_ROLES", 8), ("MAX_HEADER", 16), ("MAX_FOOTER", 8),
                      ("MAX_BOS", 8), ("MAX_GEN", 16)):
        assert re.search(r"#define SPL_CHAT_%s\s+%du\b" % (name, val), hdr), name
        assert getattr(ffi, "SPL_CHAT_" + name) == val
    sig = re.search(r"int spl_chat_device\((.*?)\);", hdr, re.S).group(1)
    assert len(re.sub(r"/\*.*?\*/", "", sig, flags=re.S).split(",")) == len(L.spl_chat_device.argtypes) == 23


def test_refusals_name_their_cause(ffi):
    """Every refusal comes before the handle or the device is touched: a dummy handle (never read) is enough, and none of the addresses
    below is ever dereferenced."""
    L = ffi.lib()
    handle = ctypes.create_string_buffer(64)
    h = ctypes.addressof(handle)
    A = 0x10000                       # an address that is aligned to everything
    O = ffi.SplChatOpts
    one = [((), ())]

    def call(t=h, ids=A, off=A, n_docs=3, turn_doc=None, turn_role=A, turn_train=None, n_turns=3, conv_off=A, n=2, o=None, rows=A, labels=A,
             loss=A, mask=A, role=A, special=A, ln=A, kept=A, turn_col=A, status=A, work=A):
        o = O(0, 8, roles=one) if o is None else o
        return L.spl_chat_device(t, ids, off, n_docs, turn_doc, turn_role, turn_train, n_turns, conv_off, n,
                                 ctypes.byref(o) if o is not False else None, rows, labels, loss, mask, role, special, ln, kept, turn_col,
                                 status, work, None)

    def refused(rc, *words):
        msg = L.spl_last_error().decode()
        assert rc == SPL_EINVAL, (rc, msg)
        for w in ("spl_chat_device",) + words:
            assert w in msg, (w, msg)

    refused(call(t=None), "null handle")
    refused(call(o=False), "options")
    refused(call(rows=None), "d_rows is null")
    refused(call(n=0, rows=None), "d_rows is null")
    refused(call(off=None), "d_off is null")
    refused(call(conv_off=None), "d_conv_off is null")
    refused(call(status=None), "d_status is null")
    refused(call(work=None), "d_work is null")
    refused(call(turn_role=None), "d_turn_role is null")
    refused(call(ids=None), "d_ids is null")
    short = O(0, 8, roles=one)
    for size in (0, 964, 4097):
        short.struct_size = size
        refused(call(o=short), "struct_size")
    refused(call(o=O(128, 8, roles=one)), "unknown flag bit 0x80")
    refused(call(o=O(0x80000000 | PAD_LEFT, 8, roles=one)), "unknown flag bit 0x80000000")
    for bit in (4, 8, 16):             # SPL_COLLATE_KEEP_TAIL, _BOS, _EOS
        refused(call(o=O(bit, 8, roles=one)), "SPL_COLLATE_KEEP_TAIL", "SPL_CHAT_DROP_OLDEST")
    refused(call(o=O(PIN_FIRST, 8, roles=one)), "SPL_CHAT_PIN_FIRST", "SPL_CHAT_DROP_OLDEST")
    for n_roles in (0, 9):
        o = O(0, 8, roles=one)
        o.n_roles = n_roles
        refused(call(o=o), "n_roles")
    for field, limit, word in (("n_bos", 8, "SPL_CHAT_MAX_BOS"), ("n_gen", 16, "SPL_CHAT_MAX_GEN")):
        o = O(0, 200, roles=one)
        setattr(o, field, limit + 1)
        refused(call(o=o), field, word)
    o = O(0, 200, roles=one * 3)
    o.n_header[2] = 17
    refused(call(o=o), "n_header[2]", "SPL_CHAT_MAX_HEADER")
    o = O(0, 200, roles=one * 3)
    o.n_footer[1] = 9
    refused(call(o=o), "n_footer[1]", "SPL_CHAT_MAX_FOOTER")
    o = O(0, 200, roles=one)
    o.n_header[1] = 99                   # (a count of a role the template does not have is not looked at)
    refused(call(o=o, rows=A + 8), "d_rows", "16-byte")
    refused(call(o=O(0, 8, roles=one * 2, train_content=4)), "train_content", "n_roles")
    refused(call(o=O(0, 8, roles=one * 2, train_footer=0x100)), "train_footer", "n_roles")
    refused(call(o=O(0, 0, roles=one)), "row_len is 0")
    refused(call(o=O(0, 3, roles=one, bos=(1, 2), gen=(3, 4))), "row_len", "bos + gen")
    refused(call(n_docs=1 << 31, turn_doc=A), "n_docs >= 2^31")
    refused(call(n_turns=1 << 31, turn_doc=A), "n_turns >= 2^31")
    refused(call(n=1 << 31), "n_convs >= 2^31")
    refused(call(n_turns=4), "d_turn_doc is null", "n_docs")
    refused(call(n=(1 << 31) - 1, o=O(0, 0xFFFFFFFF, roles=one), rows=A + 8), "d_rows", "16-byte")     # (n_convs * row_len < 2^63: never refused for its size)
    for kw, name, al in ((dict(rows=A + 8), "d_rows", "16"), (dict(labels=A + 4), "d_labels", "16"), (dict(ln=A + 4), "d_len", "16"),
                         (dict(kept=A + 8), "d_kept", "16"), (dict(turn_col=A + 8), "d_turn_col", "16"), (dict(work=A + 8), "d_work", "16"),
                         (dict(loss=A + 1), "d_loss", "4"), (dict(mask=A + 2), "d_mask", "4"), (dict(role=A + 3), "d_role", "4"),
                         (dict(special=A + 2), "d_special", "4"), (dict(turn_doc=A + 2), "d_turn_doc", "4"), (dict(conv_off=A + 4), "d_conv_off", "8")):
        refused(call(**kw), name, al + "-byte")
    # a LONGER struct is accepted and its tail ignored: the refusal that follows is about something else
    big = (ctypes.c_uint32 * 400)(1600, 0, 0)
    big[5] = 1
    refused(call(o=ctypes.cast(big, ctypes.POINTER(O)).contents), "row_len is 0")
    assert "struct_size" not in L.spl_last_error().decode()
    # nothing to do is not an error, and needs no ids, no turns and no optional output
    assert call(n=0, ids=None, n_docs=0, n_turns=0, turn_role=None, labels=None, loss=None, mask=None, role=None, special=None, ln=None,
                kept=None, turn_col=None) == 0


def test_work_bytes_monotone_and_granular(ffi, sim):
    L = ffi.lib()
    rec = sim.geometry()["rec_bytes"]
    prev_t = -1
    for n_turns in (0, 1, 2, 3, 63, 64, 65, 1000, (1 << 31) - 1):
        prev_c = -1
        for n_convs in (0, 1, 2, 5, 250, 2500, (1 << 31) - 1):
            b = int(L.spl_chat_work_bytes(n_turns, n_convs))
            assert b == sim.work_bytes(n_turns, n_convs) and b % 16 == 0 and b >= 1024 + rec * n_convs + 8 * n_turns and b > prev_c
            assert b == int(L.spl_chat_work_bytes(n_turns, n_convs))           # (a pure function)
            prev_c = b
        assert int(L.spl_chat_work_bytes(n_turns, 7)) >= prev_t          # (a turn is 8 bytes, the granule 16: two turns more always show)
        prev_t = int(L.spl_chat_work_bytes(n_turns, 7))


# ------------------------------------------------------------------------------------------ 2. the mapping code the kernels run
def _ids32(a):
    return (a & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def _compare(sim, case, tag, null=(), where=None):
    want = ref.chat_ref(*case, where=where)
    got = sim.chat(case, PAD_ID, IGNORE_ID, null=null)
    assert np.array_equal(got["rows"], _ids32(want.rows)), tag
    for name, w in (("labels", want.labels), ("loss", want.loss), ("mask", want.mask), ("role", want.role), ("special", want.special),
                    ("len", want.lens), ("kept", want.kept), ("turn_col", want.turn_col)):
        assert got[name] is None if name in null else np.array_equal(got[name], w), (name,) + tag
    assert got["status"] == want.status, tag
    return want


def test_chat_mapping_grid(sim):
    """every row length x template x flag set of chat_ref.grid; what the grid is meant to reach is asserted, not assumed"""
    cases, where, residues, dropped, pinned_full, nothing_fits, counts = 0, [], set(), 0, 0, 0, set()
    for L in ref.ROW_LENS:
        for case in ref.grid(L, 20270 + L):
            tag = (L, case.flags, len(case.tpl.roles))
            want = _compare(sim, case, tag, where=where)
            assert want.status == 0
            residues.add(case.n_convs * L % 4)
            counts |= {int(x) for x in np.diff(case.conv_off.astype(np.int64))}
            if case.flags & DROP_OLDEST:
                dropped += int((want.kept[:, 0] > 0).sum())
                nothing_fits += int(((want.kept[:, 0] > 0) & (want.kept[:, 1] > 0)).sum())
                if case.flags & PIN_FIRST:
                    pinned_full += int(((want.kept[:, 1] > 0) & (want.lens == L)).sum())
            cases += 1
    assert cases == len(ref.ROW_LENS) * 3 * len(ref.FLAG_SETS)
    assert set(ref.TURN_COUNTS) <= counts and residues == {0, 1, 2, 3}
    assert set(where) == {(part, first) for part in ("header", "content", "footer") for first in (False, True)}     # cuts inside each part and at each seam
    assert dropped > 1000 and nothing_fits > 50 and pinned_full > 20
    tpls = ref.templates(130)
    assert [len(t.roles) for t in tpls] == [1, 3, 8] and (len(tpls[2].bos), len(tpls[2].gen)) == (8, 16)
    assert {0, 16} <= {len(h) for t in tpls for h, f in t.roles} and {0, 8} <= {len(f) for t in tpls for h, f in t.roles}      # counts at 0 and at their maxima


def test_chat_mapping_optional_outputs_and_more_than_one_workgroup(sim):
    """a few hundred conversations: more than one span of the gather, more than one workgroup of the turn walk, rows that straddle lanes;
    each optional output as NULL once, and all of them at once"""
    rng = np.random.default_rng(20271)
    g = sim.geometry()
    tpl = ref.templates(65)[1]
    for n_convs, L, flags in ((300, 65, DROP_OLDEST | PIN_FIRST), (1025, 3, PAD_LEFT), (700, 7, DROP_OLDEST | PAD_LEFT)):
        tp = tpl if L >= 4 else ref.templates(L)[0]
        B = L - len(tp.bos) - len(tp.gen)
        convs = [[(int(rng.integers(0, len(tp.roles))), int(x)) for x in ref_lengths(B, int(rng.integers(0, 6)), rng)] for _ in range(n_convs)]
        case = ref.build(convs, L, flags, tp, rng, identity=False, train=True)
        assert n_convs * L > g["span"] and n_convs > g["waves"]
        _compare(sim, case, (n_convs, L, flags))
    for name in OUTPUTS:
        _compare(sim, case, ("null", name), null=(name,))
    _compare(sim, case, ("null", "all"), null=OUTPUTS)


def ref_lengths(B, n, rng):
    pool = [0, 1, 2, max(0, B // 2), max(0, B - 1), B, B + 1]
    return [pool[int(i)] for i in rng.integers(0, len(pool), size=n)]


def _case(convs, docs, L, flags, tpl, turn_train=None):
    """convs: [[(role, document index)]]; docs: lists of ids"""
    off = np.zeros(len(docs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(d) for d in docs])
    ids = np.array([x for d in docs for x in d], dtype=np.uint32)
    turns = [t for conv in convs for t in conv]
    conv_off = np.zeros(len(convs) + 1, dtype=np.uint64)
    conv_off[1:] = np.cumsum([len(c) for c in convs])
    return ref.Case(ids, off, len(docs), np.array([d for _, d in turns], dtype=np.int32), np.array([r for r, _ in turns], dtype=np.uint8),
                    None if turn_train is None else np.array(turn_train, dtype=np.uint8), len(turns), conv_off, len(convs), L, flags, tpl)


TPL2 = Template([((10, 11), (12,)), ((20, 21), (22, 23))], (1,), (20, 21), 0b10, 0b10)       # user, assistant
DOCS = [[100, 101], [200, 201, 202], [7]]


def test_drop_oldest_edges(sim):
    """nothing fits; only the last turn fits; PIN_FIRST with a single turn; PIN_FIRST with a pinned turn that alone exceeds the budget"""
    long_doc = list(range(1000, 1030))
    docs = DOCS + [long_doc]
    for pad in (0, PAD_LEFT):
        # budget 13 - 3 = 10.  nothing fits: the last turn has 2 + 30 + 1 entries -- it alone is kept and cut at 10
        case = _case([[(0, 0), (1, 1), (0, 3)]], docs, 13, DROP_OLDEST | pad, TPL2)
        want = _compare(sim, case, ("nothing fits", pad))
        assert want.kept.tolist() == [[2, 23]] and want.rows[0].tolist() == [1, 10, 11] + long_doc[:8] + [20, 21]
        assert want.turn_col.tolist() == [[-1, -1], [-1, -1], [3, 11]]
        # only the last turn fits: 5 + 7 + 5 entries against 10, then 7 + 5, then 5
        case = _case([[(0, 0), (1, 1), (0, 0)]], docs, 13, DROP_OLDEST | pad, TPL2)
        want = _compare(sim, case, ("last fits", pad))
        assert want.kept.tolist() == [[2, 0]] and want.lens.tolist() == [8]
        assert want.rows[0][want.mask[0] == 1].tolist() == [1, 10, 11, 100, 101, 12, 20, 21]
        # PIN_FIRST, a single turn: nothing to drop, the default's cut
        case = _case([[(0, 3)]], docs, 13, DROP_OLDEST | PIN_FIRST | pad, TPL2)
        want = _compare(sim, case, ("pin single", pad))
        assert want.kept.tolist() == [[0, 23]] and want.rows[0].tolist() == [1, 10, 11] + long_doc[:8] + [20, 21]
        assert np.array_equal(want.rows, ref.chat_ref(*case._replace(flags=pad)).rows)
        # PIN_FIRST, the pinned turn alone exceeds the budget: it fills the row, the last turn lies wholly behind the cut
        case = _case([[(0, 3), (1, 1), (0, 0)]], docs, 13, DROP_OLDEST | PIN_FIRST | pad, TPL2)
        want = _compare(sim, case, ("pin too long", pad))
        assert want.kept.tolist() == [[1, 28]] and want.rows[0].tolist() == [1, 10, 11] + long_doc[:8] + [20, 21]
        assert want.turn_col.tolist() == [[3, 11], [-1, -1], [-1, -1]]
        # with no turn dropped DROP_OLDEST equals the default
        case = _case([[(0, 0), (1, 1)]], docs, 16, DROP_OLDEST | PIN_FIRST | pad, TPL2)
        want = _compare(sim, case, ("fits", pad))
        plain = ref.chat_ref(*case._replace(flags=pad))
        assert all(np.array_equal(a, b) for a, b in zip(want[:-1], plain[:-1])) and want.kept.tolist() == [[0, 0]]


def test_bad_roles_documents_and_ranges(sim):
    seen = 0
    for L in (5, 64):
        for i, case in enumerate(ref.grid(L, 20272 + L)):
            kind = ref.BAD_KINDS[i % len(ref.BAD_KINDS)]
            bad = ref.spoil(case, kind)
            want = _compare(sim, bad, (L, kind, case.flags))
            assert want.status == 1, (L, kind)
            if kind.startswith("range"):                # the last conversation has no turns: its row is bos + gen, its turns are not written
                assert want.lens[-1] == len(case.tpl.bos) + len(case.tpl.gen)
                first = int(case.conv_off[-2])
                assert first == case.n_turns or (want.turn_col[first:] == ref.UNWRITTEN).all()
            seen += 1
    assert seen >= 2 * len(ref.BAD_KINDS)


def test_index_arithmetic_beyond_2_to_32(sim):
    """Rows of 2^31 - 1 entries (the longest whose columns fit d_turn_col's int32), three conversations: flat indices pass 2^32.  No memory holds such an output: single groups of the
    gather's mapping are evaluated where something happens -- the rows' starts and ends -- and compared with a row built by hand."""
    L, n = (1 << 31) - 1, 3
    convs = [[(0, 0), (1, 1)], [], [(1, 1), (0, 2), (1, 0)]]
    total = n * L
    assert total > (1 << 32) and total % 4 == 1
    for flags in (0, PAD_LEFT | DROP_OLDEST):
        case = _case(convs, DOCS, L, flags, TPL2)
        small = ref.chat_ref(*case._replace(L=64))               # (nothing is cut at 64 either: the rows are these, with more padding)
        e0 = sorted({e for p in range(n + 1) for e in range(max(0, (p * L - 40) // 4 * 4), min(total, p * L + 44), 4)})
        assert e0[-1] + 1 == total and sum(e > (1 << 32) for e in e0) > 10
        v, bits, roles, lens, kept, tc, status = sim.groups(case, PAD_ID, IGNORE_ID, e0)
        assert lens.tolist() == small.lens.tolist() and kept.tolist() == [[0, 0]] * 3 and status == 0
        for g, e in enumerate(e0):
            for i in range(4):
                if e + i >= total:
                    assert v[g, i] == PAD_ID and bits[g, i] == 0
                    continue
                p, c = divmod(e + i, L)
                used = int(small.lens[p])
                j = c - (L - used) if flags & PAD_LEFT else c
                s = j + (64 - used if flags & PAD_LEFT else 0)          # the same entry's column in the small rows
                if 0 <= j < used:
                    want = (int(small.rows[p, s]), 1 | 2 * int(small.loss[p, s]) | 4 * int(small.special[p, s]), int(small.role[p, s]))
                else:
                    want = (PAD_ID, 4, 255)
                assert (int(v[g, i]), int(bits[g, i]), int(roles[g, i])) == want, (flags, e, i, p, c)
        shift = (L - 64) if flags & PAD_LEFT else 0
        assert tc.tolist() == [[a + shift, b + shift] for a, b in small.turn_col.tolist()]


# ------------------------------------------------------------------------------------------ 3. chat_ref against hand-written examples
def test_ref_two_turns_by_hand():
    case = _case([[(0, 0), (1, 1)]], DOCS, 16, 0, TPL2)
    out = ref.chat_ref(*case, pad_id=0)
    assert out.rows.tolist() == [[1, 10, 11, 100, 101, 12, 20, 21, 200, 201, 202, 22, 23, 20, 21, 0]]
    assert out.labels.tolist() == [[-100] * 8 + [200, 201, 202, 22, 23] + [-100] * 3]
    assert out.loss.tolist() == [[0] * 8 + [1] * 5 + [0] * 3] and out.mask.tolist() == [[1] * 15 + [0]]
    assert out.role.tolist() == [[255, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 255, 255, 255]]
    assert out.special.tolist() == [[1, 1, 1, 0, 0, 1, 1, 1, 0, 0, 0, 1, 1, 1, 1, 1]]
    assert out.lens.tolist() == [15] and out.kept.tolist() == [[0, 0]] and out.turn_col.tolist() == [[3, 5], [8, 11]] and out.status == 0
    # the footer of a trained role is not trained without its bit; a turn with turn_train == 0 carries no labels at all
    out = ref.chat_ref(*case._replace(tpl=TPL2._replace(train_footer=0)), pad_id=0)
    assert out.labels.tolist() == [[-100] * 8 + [200, 201, 202] + [-100] * 5]
    out = ref.chat_ref(*case._replace(turn_train=np.array([1, 0], dtype=np.uint8)), pad_id=0)
    assert (out.labels == -100).all() and not out.loss.any()


def test_ref_cut_and_drop_by_hand():
    # budget 10 - 3 = 7 against a body of 5 + 7
    case = _case([[(0, 0), (1, 1)]], DOCS, 10, 0, TPL2)
    out = ref.chat_ref(*case, pad_id=0)
    assert out.rows.tolist() == [[1, 10, 11, 100, 101, 12, 20, 21, 20, 21]]           # the cut falls between the second header and its content
    assert out.kept.tolist() == [[0, 5]] and out.turn_col.tolist() == [[3, 5], [-1, -1]] and (out.labels == -100).all()
    out = ref.chat_ref(*case._replace(flags=DROP_OLDEST), pad_id=0)
    assert out.rows.tolist() == [[1, 20, 21, 200, 201, 202, 22, 23, 20, 21]]
    assert out.kept.tolist() == [[1, 0]] and out.turn_col.tolist() == [[-1, -1], [3, 6]]
    assert out.labels.tolist() == [[-100] * 3 + [200, 201, 202, 22, 23] + [-100] * 2]
    out = ref.chat_ref(*case._replace(L=9), pad_id=0)                                   # budget 6: the cut falls inside the second header
    assert out.rows.tolist() == [[1, 10, 11, 100, 101, 12, 20, 20, 21]] and out.kept.tolist() == [[0, 6]]


def test_ref_pinned_shared_and_bad_by_hand():
    tpl = Template([((10, 11), (12,)), ((20, 21), (22, 23)), ((30,), (31,))], (1,), (), 0b10, 0b10)      # user, assistant, system
    convs = [[(2, 2), (0, 0), (1, 1), (0, 0)], [(1, 9)]]                   # the user's message twice: ONE document; document 9 does not exist
    case = _case(convs, DOCS, 14, DROP_OLDEST | PIN_FIRST | PAD_LEFT, tpl)
    out = ref.chat_ref(*case, pad_id=0)
    # budget 13: 3 + (5 + 7 + 5), 3 + (7 + 5), then 3 + 5 fits
    assert out.rows[0].tolist() == [0] * 5 + [1, 30, 7, 31, 10, 11, 100, 101, 12]
    assert out.rows[1].tolist() == [0] * 9 + [1, 20, 21, 22, 23]
    assert out.kept.tolist() == [[2, 0], [0, 0]] and out.lens.tolist() == [9, 5] and out.status == 1
    assert out.turn_col.tolist() == [[7, 8], [-1, -1], [-1, -1], [11, 13], [-1, -1]]
    assert (out.labels[0] == -100).all() and out.labels[1].tolist() == [-100] * 12 + [22, 23]
    assert out.role[0].tolist() == [255] * 6 + [2, 2, 2, 0, 0, 0, 0, 0] and out.special[0].tolist() == [1] * 7 + [0, 1, 1, 1, 0, 0, 1]


# ------------------------------------------------------------------------------------------ 4. the built-in templates
CONVS = [
    [("system", "You are a helpful assistant."), ("user", "What is 2 + 2?"), ("assistant", "4"), ("user", "And 3 + 3?"), ("assistant", "6 it is.\n")],
    [{"role": "user", "content": "你好世界"}, {"role": "assistant", "content": "Hello 🌍 World! "}],
    [("user", ""), ("assistant", "a"), ("tool_or_ipython", "42 results\n\n"), ("assistant", "Done")],
    [("system", "x" * 40), ("user", "naïve café?   ")],
    [],
]


def _special(name):
    with open(os.path.join(ROOT, "splintr_amd", "data", "special_tokens.json"), encoding="utf-8") as f:
        return json.load(f)[name]


def _oracle_case(orc, tpl, convs, L, flags=0):
    from splintr_amd.device import chat_turns
    texts, turn_doc, turn_role, turn_train, conv_off = chat_turns(convs, tpl)
    docs = orc.encode_batch(texts) if texts else []
    T = Template(list(tpl.roles.values()), tpl.bos, tpl.generation if flags & 0x1000 else (), tpl.train_content_mask, tpl.train_footer_mask)
    off = np.zeros(len(docs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(d) for d in docs])
    return ref.Case(np.array([x for d in docs for x in d], dtype=np.uint32), off, len(docs), turn_doc, turn_role, turn_train, len(turn_doc),
                    conv_off.astype(np.uint64), len(convs), L, flags & ~0x1000, T)


@pytest.mark.parametrize("fmt,name", [("chatml", "cl100k_base"), ("llama3", "llama3"), ("chatml", "llama3")])
def test_templates_equal_the_rendered_string(coracle, fmt, name):
    """bos + turns (+ the generation prompt) built from separately encoded messages == the oracle's encode_with_special of the rendered
    string, for every conversation whose contents begin with a letter or a digit (or are empty); none is skipped"""
    from splintr_amd.chat import ChatTemplate
    orc = coracle(name)
    tpl = getattr(ChatTemplate, fmt)(orc, _special(name))
    fourth = list(tpl.roles)[3]
    assert fourth == ("tool" if fmt == "chatml" else "ipython") and list(tpl.roles)[:3] == ["system", "user", "assistant"]
    convs = [[(fourth if (m["role"] if isinstance(m, dict) else m[0]) == "tool_or_ipython" else (m["role"] if isinstance(m, dict) else m[0]),
               m["content"] if isinstance(m, dict) else m[1]) for m in conv] for conv in CONVS]
    checked = 0
    for gen in (False, True):
        case = _oracle_case(orc, tpl, convs, 256, 0x1000 if gen else 0)
        out = ref.chat_ref(*case)
        assert out.status == 0 and (out.kept == 0).all()
        for c, conv in enumerate(convs):
            assert all(m[1] == "" or m[1][0].isalnum() for m in conv)
            want = orc.encode_with_special(tpl.render(conv, add_generation_prompt=gen))
            assert out.rows[c, :out.lens[c]].tolist() == want, (fmt, name, c, gen)
            checked += 1
        # labels: exactly the assistant's content and footer
        asst = tpl.role_of("assistant")
        n_h = len(tpl.roles["assistant"][0])
        for c in range(len(convs)):
            in_turn = out.role[c] == asst
            trained = out.loss[c] == 1
            assert not (trained & ~in_turn).any()
            assert (out.labels[c][trained] == out.rows[c][trained].astype(np.int64)).all() and (out.labels[c][~trained] == -100).all()
        t_asst = [t for t in range(case.n_turns) if case.turn_role[t] == asst]
        assert int(out.loss.sum()) == sum(int(case.off[d + 1] - case.off[d]) for d in (int(case.turn_doc[t]) for t in t_asst)) + \
            len(t_asst) * len(tpl.roles["assistant"][1]) and n_h > 0
    assert checked == 2 * len(CONVS)


def test_llama3_seam_convention_is_pinned(coracle):
    """a content that begins with newlines joins the header's "\\n\\n" in the rendered string; encoded turn by turn it does not: the ids
    DIFFER, and the row holds the message's own ids"""
    from splintr_amd.chat import ChatTemplate
    orc = coracle("llama3")
    tpl = ChatTemplate.llama3(orc, _special("llama3"))
    conv = [("user", "\n\nx")]
    case = _oracle_case(orc, tpl, [conv], 64)
    out = ref.chat_ref(*case)
    row = out.rows[0, :out.lens[0]].tolist()
    rendered = orc.encode_with_special(tpl.render(conv))
    assert row != rendered
    c0, c1 = out.turn_col[0].tolist()
    assert row[c0:c1] == orc.encode("\n\nx") and row[:c0] == list(tpl.bos) + list(tpl.roles["user"][0])
    eot = _special("llama3")["<|eot_id|>"]
    assert row[c1:] == [eot] == list(tpl.roles["user"][1])


def test_template_errors():
    from splintr_amd.chat import ChatTemplate

    class Enc:
        def encode(self, s):
            return [ord(ch) for ch in s]
    with pytest.raises(ValueError, match=r"<\|im_start\|>"):
        ChatTemplate.chatml(Enc(), {"<|im_end|>": 5})
    with pytest.raises(ValueError, match=r"<\|eot_id\|>"):
        ChatTemplate.llama3(Enc(), {"<|begin_of_text|>": 1, "<|start_header_id|>": 2, "<|end_header_id|>": 3})
    t = ChatTemplate.chatml(Enc(), {"<|im_start|>": 1000, "<|im_end|>": 1001})
    assert t.roles["user"] == ((1000, 117, 115, 101, 114, 10), (1001, 10)) and t.generation == t.roles["assistant"][0] and t.bos == ()
    assert t.train_content_mask == 4 and t.train_footer_mask == 4 and t.role_of("tool") == 3
    assert t.render([("user", "hi")], True) == "<|im_start|>user\nhi<|im_end|>\n<|im_start|>assistant\n"
    assert ChatTemplate.chatml(Enc(), {"<|im_start|>": 1, "<|im_end|>": 2}, train=("assistant", "tool"), train_footer=False).train_footer_mask == 0
    for kw, word in ((dict(roles={}), "roles"), (dict(roles={"a": ([1] * 17, [])}), "header"), (dict(roles={"a": ([], [1] * 9)}), "footer"),
                     (dict(roles={"a": ([], [])}, bos=[1] * 9), "bos"), (dict(roles={"a": ([], [])}, generation=[1] * 17), "generation"),
                     (dict(roles={"a": ([-1], [])}), "32 bits"), (dict(roles={"a": ([], [])}, train=("b",)), "train"),
                     (dict(roles={str(i): ([], []) for i in range(9)}), "roles")):
        kw.setdefault("train", ())
        with pytest.raises(ValueError, match=word):
            ChatTemplate(**kw)
    with pytest.raises(ValueError, match="unknown role"):
        t.render([("wizard", "hi")])
    with pytest.raises(ValueError, match="no string form"):
        ChatTemplate({"a": ([1], [2])}, train=()).render([])


# ------------------------------------------------------------------------------------------ 5. the Python surface refuses before it works
def test_check_chat_args_and_chat_turns():
    import torch
    from splintr_amd.chat import ChatTemplate
    from splintr_amd.device import chat_turns, check_chat_args
    t = ChatTemplate({"user": ([1], [2]), "assistant": ([3, 4], [5])}, bos=[9], generation=[3, 4])
    check_chat_args(8, 0, t)
    check_chat_args(3, 0xFFFFFFFF, t, True, "drop_oldest", True, "left", -100, torch.int64)
    for kw, word in ((dict(dtype=torch.int16), "dtype"), (dict(truncation="left"), "truncation"), (dict(pin_system=True), "pin_system"),
                     (dict(padding_side="both"), "padding_side"), (dict(ignore_index=1 << 32), "ignore_index"),
                     (dict(ignore_index=-(1 << 31) - 1), "ignore_index")):
        with pytest.raises(ValueError, match=word):
            check_chat_args(8, 0, t, **kw)
    with pytest.raises(ValueError, match="pad_id"):
        check_chat_args(8, 1 << 32, t)
    with pytest.raises(ValueError, match="template"):
        check_chat_args(8, 0, {"user": ([1], [2])})
    with pytest.raises(ValueError, match="row length"):
        check_chat_args(0, 0, t)
    with pytest.raises(ValueError, match="row length"):
        check_chat_args(2, 0, t, True)
    check_chat_args(1, 0, t)
    convs = [[("user", "hi"), ("assistant", "sys")], [{"role": "user", "content": "sys"}, ("assistant", "hi"), ("user", "hi")], []]
    texts, turn_doc, turn_role, turn_train, conv_off = chat_turns(convs, t)
    assert texts == ["hi", "sys"] and turn_doc.tolist() == [0, 1, 1, 0, 0] and turn_role.tolist() == [0, 1, 0, 1, 0]       # equal strings: ONE document
    assert turn_train is None and conv_off.tolist() == [0, 2, 5, 5]
    assert chat_turns(convs, t, [[1, 0], [0, 1, 1], []])[3].tolist() == [1, 0, 0, 1, 1]
    for bad, word in (("a string", "conversations"), ([("user", "hi")], "message"), ([[("user", "hi")], 5], "conversation 1"), ([[("user",)]], "message"), ([[("wizard", "x")]], "unknown role"),
                      ([[{"role": "user"}]], "content"), ([[("user", b"x")]], "str")):
        with pytest.raises(ValueError, match=word):
            chat_turns(bad, t)
    with pytest.raises(ValueError, match="train_turns"):
        chat_turns(convs, t, [[1, 0]])


def test_encode_batch_chat_validates_before_anything_goes_to_the_device():
    """Bad arguments raise ValueError BEFORE the messages are packed, uploaded or encoded: a tokenizer object without a handle is enough."""
    import torch
    from splintr_amd import Tokenizer
    from splintr_amd.chat import ChatTemplate
    t = Tokenizer.__new__(Tokenizer)
    tpl = ChatTemplate({"user": ([1], [2]), "assistant": ([3], [4])})
    convs = [[("user", "hi")]]
    with pytest.raises(ValueError, match="dtype"):
        t.encode_batch_chat(convs, 8, template=tpl, pad_id=0, dtype=torch.float32)
    with pytest.raises(ValueError, match="truncation"):
        t.encode_batch_chat(convs, 8, template=tpl, pad_id=0, truncation="oldest")
    with pytest.raises(ValueError, match="pin_system"):
        t.encode_batch_chat(convs, 8, template=tpl, pad_id=0, pin_system=True)
    with pytest.raises(ValueError, match="template"):
        t.encode_batch_chat(convs, 8, template=None, pad_id=0)
    with pytest.raises(ValueError, match="unknown role"):
        t.encode_batch_chat([[("system", "hi")]], 8, template=tpl, pad_id=0)
    with pytest.raises(ValueError, match="conversations"):
        t.encode_batch_chat("one string", 8, template=tpl, pad_id=0)
