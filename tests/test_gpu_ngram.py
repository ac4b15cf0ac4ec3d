"""GPU tests (-m gpu): spl_ngram_draft_device -- n-gram drafting -- into guarded buffers, bit for bit against the definition of
tests/ngram_ref.py: lengths around the tile and slice edges, one to three slices, the options, holes, the tail and its append, batch
sizes, every refusal by its message, and a speculative loop end to end beside a plain guided loop."""
import ctypes
import random

import numpy as np
import pytest

import vocabgen
from ngram_ref import ngram_ref

pytestmark = pytest.mark.gpu

CAP, POISON, PAD = 2304, 0x5A5A5A5A, 7
FIELDS = ("ids", "count", "match", "from_", "parent")
_tok, _refs = [], {}


@pytest.fixture(scope="module")
def tok(tmp_path_factory):
    from splintr_amd import Tokenizer
    enc = {bytes([b]): b for b in range(256)}
    enc.update({b"ab": 256, b"cd": 257, b"abc": 258})
    path = tmp_path_factory.mktemp("ngram") / "toy.tiktoken"
    path.write_bytes(vocabgen.tiktoken(enc))
    yield Tokenizer(str(path), r"[a-z]+|\s+|[^a-z\s]+", {"<|end|>": 300})
    import gc
    import torch
    gc.collect()
    torch.cuda.synchronize()


def _history(alpha, L, cap, seed, dtype=np.int32):
    """a row of cap ids over `alpha` symbols, the same law behind L as in front of it (a read beyond L would find matches there); the
    50-symbol rows get the row's last 6 ids planted across position 1024 and across 2048, where tiles and slices meet"""
    rng = random.Random(seed)
    row = [rng.randrange(alpha) for _ in range(cap)]
    if alpha == 50 and L >= 6:
        for edge in (1024, 2048):
            if edge + 3 < L - 6:
                row[edge - 3:edge + 3] = row[L - 6:L]
    return np.array(row, dtype=dtype)


def _run(tok, rows, lens, new=None, new_len=None, *, slices=0, pick="latest", **o):
    """one call into guarded buffers -> what it wrote, as numpy; nothing beside the rows may change, nor any input but hist"""
    import torch
    from splintr_amd import device as dv
    dev = torch.device("cuda", 0)
    B, cap = rows.shape
    tdt = torch.int64 if rows.dtype == np.int64 else torch.int32
    W = max(o["branches"] * o["depth"], 1)

    def guarded(w, dt=torch.int32):
        return torch.full((B + 1, w), 0x5A if dt == torch.uint8 else POISON, dtype=dt, device=dev)

    big = guarded(cap, tdt)
    big[:B] = torch.from_numpy(rows).to(dev)
    t_len = torch.tensor(lens, dtype=torch.int32, device=dev)
    t_new = None if new is None else torch.from_numpy(np.ascontiguousarray(new)).to(dev)
    t_nl = None if new is None else torch.tensor(new_len, dtype=torch.int32, device=dev)
    bufs = dict(ids=guarded(W, tdt), count=guarded(o["branches"]), match=guarded(o["branches"]), from_=guarded(o["branches"]), parent=guarded(W),
                length=guarded(1), full=guarded(1, torch.uint8))
    out = dv.NgramDraft(*(bufs[k][:B] for k in FIELDS))
    dv.ngram_draft_device(tok, big[:B], t_len, new=t_new, new_len=t_nl, slices=slices, pick=pick, pad_id=PAD, out=out, out_lengths=bufs["length"][:B, 0],
                          full=bufs["full"][:B, 0], **o)
    torch.cuda.synchronize()
    bufs["hist"] = big
    for k, t in bufs.items():
        assert (t[B] == (0x5A if t.dtype == torch.uint8 else POISON)).all().item(), f"{k}: the row behind the last was written"
    assert t_len.cpu().tolist() == list(lens) and (new is None or (np.array_equal(t_new.cpu().numpy(), new) and t_nl.cpu().tolist() == list(new_len)))
    return {k: t[:B].cpu().numpy() for k, t in bufs.items()}


def _check(tok, key, rows, lens, new=None, new_len=None, *, slices=0, pick="latest", **o):
    """the call against the reference (computed once per key, shared among the slice counts) -> the reference's rows"""
    B, cap = rows.shape
    if key not in _refs:
        _refs[key] = [ngram_ref(rows[b].tolist(), lens[b], [] if new is None else new[b].tolist(), 0 if new is None else new_len[b], cap,
                                earliest=pick == "earliest", pad_id=PAD, **o) for b in range(B)]
    got = _run(tok, rows, lens, new, new_len, slices=slices, pick=pick, **o)
    for b, want in enumerate(_refs[key]):
        assert got["hist"][b].tolist() == want["hist"], (b, "hist")
        assert (int(got["length"][b, 0]), int(got["full"][b, 0])) == (want["length"], want["full"]), b
        for k in FIELDS:
            if o["depth"]:
                assert got[k][b].tolist() == want[k], (b, k, lens[b], got["from_"][b].tolist(), want["from_"])
            else:
                assert (got[k][b] == POISON).all(), (b, k)
    return _refs[key]


LENGTHS = (0, 1, 2, 3, 1023, 1024, 1025, 2047, 2049, 2300)                     # (min_n = 2: L = min_n and min_n + 1 are among them)


@pytest.mark.parametrize("slices", [1, 2, 3])
@pytest.mark.parametrize("alpha", [2, 3, 50])
def test_lengths_around_every_edge(tok, alpha, slices):
    rows = np.stack([_history(alpha, L, CAP, 100 * alpha + i) for i, L in enumerate(LENGTHS)])
    want = _check(tok, ("edge", alpha), rows, LENGTHS, slices=slices, min_n=2, max_n=4, depth=8, branches=4)
    if alpha == 2:                                                                # two symbols: exactly two branches, the rest empty
        for w in want[4:]:
            assert [c > 0 for c in w["count"]] == [True, True, False, False] and w["from_"][2:] == [-1, -1] and set(w["parent"][16:]) == {-2}
    if alpha == 50:                                                               # the planted repeats are found across the edges
        assert want[8]["from_"][0] == 1027 and want[9]["from_"][0] == 2051 and want[9]["match"][0] == 4


SHAPES = [(1, 1), (1, 4), (1, 8), (8, 1), (8, 4), (8, 8), (64, 1)]


@pytest.mark.parametrize("dtype,pick", [(np.int32, "latest"), (np.int64, "earliest"), (np.int64, "latest"), (np.int32, "earliest")])
@pytest.mark.parametrize("depth,branches", SHAPES)
@pytest.mark.parametrize("min_n,max_n", [(1, 1), (2, 4), (3, 8)])
def test_options(tok, min_n, max_n, depth, branches, dtype, pick):
    lens = (1100, 1029, 1500, 900)
    rows = np.stack([_history(a, L, 1536, 7 * a, dtype) for a, L in zip((2, 3, 10, 50), lens)])
    want = _check(tok, ("opt", min_n, max_n, depth, branches, dtype, pick), rows, lens, pick=pick, min_n=min_n, max_n=max_n, depth=depth, branches=branches)
    if min_n == 1:                                                                # ten symbols, 1 500 ids: every branch exists -- and is full, the latest end's apart
        assert all(want[2]["count"]) and (pick == "latest" or want[2]["count"] == [depth] * branches)


def test_holes(tok):
    big = 1 << 31
    rows = np.full((6, 64), -1, dtype=np.int64)
    seqs = [[1, 2, 3, 9, 9, 1, -1, 3],             # a hole inside the suffix: matches of length 1 only
            [1, -1, 3, 4, 5, 1, 2, 3],             # a hole inside a would-be match: 2 3 is not there, 3 alone is
            [1, 2, 3, -1, 8, 2, 3, 6, 1, 2, 3],    # a hole as H[e]: the longer match is skipped, the shorter taken
            [1, 2, 3, 4, big, 5, 9, 1, 2, 3],      # a hole inside the continuation cuts the branch; 2^31 is one
            [big, 5, big],                         # a hole equals nothing, not even itself
            [4, 5, 6, 7, 4, 5, big - 1, 4, 5]]     # 2^31 - 1 is an id
    for b, s in enumerate(seqs):
        rows[b, :len(s)] = s
    want = _check(tok, "holes", rows, [len(s) for s in seqs], min_n=1, max_n=3, depth=4, branches=2)
    assert [(w["match"][0], w["from_"][0], w["count"][0]) for w in want] == [(1, 3, 3), (1, 3, 4), (2, 7, 4), (3, 3, 1), (0, -1, 0), (2, 6, 3)]


@pytest.mark.parametrize("slices", [1, 3])
def test_the_tail_and_its_append(tok, slices):
    lens = [1022, 1030, CAP - 3, 300, -5]                                         # the tail across a tile edge, across cap, a negative length
    rows = np.stack([_history(3, max(L, 0), CAP, 31 + i) for i, L in enumerate(lens)])
    new = np.stack([_history(3, 8, 8, 41 + i) for i in range(5)])
    for nl in ([0, 0, 0, 0, 0], [1, 1, 1, 1, 1], [5, 5, 5, 9, 5]):
        want = _check(tok, ("tail", tuple(nl)), rows, lens, new, nl, slices=slices, min_n=2, max_n=4, depth=8, branches=2)
        assert [w["full"] for w in want] == [0, 0, int(nl[2] > 3), 0, 0] and want[2]["length"] == min(CAP, CAP - 3 + nl[2])
    assert want[0]["from_"][0] + want[0]["count"][0] > 1022                      # (five new ids: the first draft's continuation lies partly in `new`)
    fill = np.stack([_history(50, 2000, 2000, 51 + i) for i in range(5)])         # depth 0: a 2 000-id prompt is appended, no draft is written
    _check(tok, "fill", rows, [0, 5, 400, CAP, 1024], fill, [2000, 2000, 1999, 2000, 7], slices=slices, min_n=2, max_n=4, depth=0, branches=1)


@pytest.mark.parametrize("B,cap", [(1, 1301), (3, 2050), (65, 1301)])
def test_batch_sizes_and_rows_off_16_bytes(tok, B, cap):
    lens = [(37 * b * b + 11) % (cap + 1) for b in range(B)]
    rows = np.stack([_history(2 + b % 3, L, cap, b) for b, L in enumerate(lens)])
    _check(tok, ("batch", B, cap), rows, lens, slices=2 if B == 3 else 0, min_n=2, max_n=4, depth=8, branches=1)


def test_refusals(tok):
    import torch
    from splintr_amd import _ffi
    dev = torch.device("cuda", 0)
    t = {k: torch.full((64,), POISON, dtype=torch.int32, device=dev) for k in ("hist", "len", "new", "nl", "ids", "count", "match", "from_", "parent", "olen")}
    p = {k: v.data_ptr() for k, v in t.items()}
    L = _ffi.lib()

    def call(si=None, o=None, so=None, msg=""):
        size = (si or {}).pop("size", None)
        si = dict(dict(n_seqs=2, cap=16, hist=p["hist"], lengths=p["len"], new=p["new"], new_len=p["nl"], new_row_len=4), **(si or {}))
        o = dict(dict(flags=0, min_n=2, max_n=4, depth=4, branches=2, pad_id=0, slices=0), **(o or {}))
        so = dict(dict(ids=p["ids"], count=p["count"], match=p["match"], from_=p["from_"], parent=p["parent"], lengths=p["olen"], full=None), **(so or {}))
        a, b, c = _ffi.SplNgramIn(**si), _ffi.SplNgramOpts(**o), _ffi.SplNgramOut(**so)
        if size is not None:
            a.struct_size = size
        assert L.spl_ngram_draft_device(tok.handle, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), None) == -1 and msg in _ffi.last_error(), _ffi.last_error()

    call(si=dict(hist=None), msg="d_hist is null")
    call(si=dict(lengths=None), msg="d_len is null")
    call(so=dict(lengths=None), msg="the output d_len is null")
    call(so=dict(count=None), msg="d_ids, d_count, d_match or d_from is null")
    call(so=dict(parent=None), msg="more than one branch without d_parent")
    call(si=dict(new_len=None), msg="d_new and d_new_len come together")
    call(si=dict(size=8), msg="spl_ngram_in.struct_size is not set")
    call(si=dict(size=5000), msg="spl_ngram_in.struct_size is not set")
    call(o=dict(flags=4), msg="unknown flag bit 0x4")
    for bad in (dict(min_n=0), dict(min_n=5), dict(max_n=9)):
        call(o=bad, msg="are not 1 <= min_n <= max_n <= SPL_NGRAM_MAX_N (8)")
    call(o=dict(depth=65, branches=1), msg="above SPL_NGRAM_MAX_DEPTH (64)")
    call(o=dict(branches=9), msg="not in 1 .. SPL_NGRAM_MAX_BRANCHES (8)")
    call(o=dict(branches=0), msg="not in 1 .. SPL_NGRAM_MAX_BRANCHES (8)")
    call(o=dict(depth=33), msg="branches * depth is 66, above SPL_DRAFT_MAX_NODES (64)")
    call(o=dict(slices=33), msg="above SPL_NGRAM_MAX_SLICES (32)")
    call(si=dict(cap=(1 << 24) + 1), msg="above SPL_NGRAM_MAX_CAP")
    call(si=dict(n_seqs=1 << 31), msg="n_seqs >= 2^31")
    call(si=dict(hist=p["hist"] + 4), o=dict(flags=1), msg="not aligned to its element type")
    call(so=dict(count=p["count"] + 2), msg="an int32 array is not 4-byte aligned")
    call(so=dict(ids=p["hist"]), msg="d_ids coincides with an input array")
    call(so=dict(count=p["len"]), msg="d_count coincides with an input array")
    call(so=dict(lengths=p["nl"]), msg="the output d_len coincides with an input array")
    call(so=dict(match=p["count"]), msg="d_match coincides with d_count")
    call(si=dict(new=p["hist"] + 64), msg="d_new overlaps d_hist")
    torch.cuda.synchronize()
    assert all((v == POISON).all().item() for v in t.values()), "a refused call wrote something"
    with pytest.raises(ValueError, match="pick must be"):
        tok.ngram_drafter(2, 64, pick="best")


def test_speculative_loop_end_to_end(tok):
    """a greedy "model" whose logits depend on the last id alone, under a regex guide: drafting with NgramDrafter, verifying with
    guide.draft and committing with accept emits the plain guided loop's ids, in no more forward passes"""
    import torch
    dev = torch.device("cuda", 0)
    B, T, K, END = 4, 40, 6, 300
    plain = tok.regex_guide(B, r"[a-h]+", end_ids=[END])
    V = 32 * plain.n_words
    table = torch.randn((V, V), generator=torch.Generator().manual_seed(5)).to(dev)
    table[:, END] = -1e9
    start = torch.tensor([97, 98, 99, 100], dtype=torch.int32, device=dev)

    def greedy(guide, last, mask):                                                # last [R] -> the model's id behind each, under the mask's rows
        logits = table[last.long()].contiguous()
        guide.apply(logits, mask=mask.reshape(-1, mask.shape[-1]).contiguous())
        return logits.argmax(1).to(torch.int32)

    plain.begin()
    last, want = start, []
    for _ in range(T):
        last = greedy(plain, last, plain.mask)
        plain.step(last)
        want.append(last.cpu().tolist())
    want = [[w[b] for w in want] for b in range(B)]

    guide = tok.regex_guide(B, r"[a-h]+", end_ids=[END])
    guide.begin()
    drafter = tok.ngram_drafter(B, 256, min_n=1, max_n=4, depth=K)
    drafter.begin(start.view(B, 1))
    got, fed, count, passes, accepted = [[] for _ in range(B)], None, None, 0, 0
    rows = torch.arange(B, device=dev)
    while min(map(len, got)) < T:
        d = drafter.step(fed, count)
        v = guide.draft(d.ids, d.lengths)
        prev = torch.cat([(start if fed is None else fed[rows, (count - 1).long()]).view(B, 1), d.ids], 1)          # the id in front of every row
        model = greedy(guide, prev.reshape(-1), v.mask).view(B, 1 + K)            # ONE forward pass over the root and the draft
        passes += 1
        agree = (model[:, :K] == d.ids) & (torch.arange(K, device=dev) < d.lengths.view(B, 1)) & v.ok.bool()
        n = agree.to(torch.int32).cumprod(1).sum(1)
        fed = torch.cat([d.ids, torch.zeros((B, 1), dtype=torch.int32, device=dev)], 1)
        fed[rows, n.long()] = model[rows, n.long()]
        count = (n + 1).to(torch.int32)
        guide.accept(fed, count)
        accepted += int(n.sum())
        for b, (row, c) in enumerate(zip(fed.cpu().tolist(), count.cpu().tolist())):
            got[b] += row[:c]
    assert [g[:T] for g in got] == want
    assert passes <= T and accepted > 0, (passes, accepted)
