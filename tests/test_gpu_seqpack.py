"""GPU tests (-m gpu) of spl_seqpack_device (csrc/spl_k_seqpack.h): whole sequences binned into rows, none cut in two.

Expected values: tests/seqpack_ref.py (plain loops, written from the header's semantics); end to end the rows that go in come from
chat_device and from the oracle.  The grid is test_seqpack_cpu.py's (seqpack_sim.grid_cases / shaped_cases).  Every output the kernels
write -- the work buffer included -- is a view INSIDE one allocation with guard elements in front and behind it, filled with a sentinel
like the view itself (test_gpu_collate.Guarded): each check asserts that the guards are untouched; an element the kernels skipped shows
as the sentinel in the comparison.  Shapes are tiny: rows of 1..130 entries, at most a few thousand sequences."""
import ctypes

import numpy as np
import pytest

import seqpack_ref as ref
from test_gpu_collate import SENT, Guarded, _dev, _stream
from test_gpu_parity import tok

pytestmark = pytest.mark.gpu

NAME = "cl100k_base"
STRATEGIES = ("next_fit", "best_fit_decreasing")
FILLS = (1, 2, 3, 255)


@pytest.fixture(scope="module")
def sim():
    import seqpack_sim
    return seqpack_sim


def _upload(inp):
    """the case's input arrays on the device; each with one element behind it, so that none is ever a null pointer"""
    import torch
    up = lambda a: None if a is None else torch.from_numpy(np.concatenate([a.reshape(-1), np.zeros(4, dtype=a.dtype)])).to(_dev())
    return dict(ids=up(inp.ids), lengths=up(inp.lengths), off=None if inp.off is None else up(inp.off.astype(np.int64)), lab=up(inp.lab),
                byt=[up(b) for b in inp.byt])


def _pack(t, sim, inp, d, L, strategy, want, *, max_rows=None, keep_tail=False, mask_first=True, null=()):
    """one spl_seqpack_device call into guarded buffers, compared with want = seqpack_ref.pack(...)"""
    import torch
    from splintr_amd import _ffi
    lib = _ffi.lib()
    n = inp.n
    R = n if max_rows is None else max_rows
    dt = torch.int64 if inp.i64 else torch.int32
    g = {"rows": Guarded(R * L, dt), "labels": Guarded(R * L, dt), "mask": Guarded(R * L, torch.uint8), "pos": Guarded(R * L, torch.int32),
         "sid": Guarded(R * L, torch.int32), "place": Guarded(2 * n, torch.int32), "fill": Guarded(R, torch.int32),
         "cu": Guarded(n + R + 1, torch.int32), "n": Guarded(4, torch.int64), "status": Guarded(1, torch.int32),
         "work": Guarded(int(lib.spl_seqpack_work_bytes(n, R, ref.STRATEGIES[strategy])), torch.uint8)}
    for k in range(4):
        g[f"b{k}"] = Guarded(R * L, torch.uint8)
    if want.status:
        g["status"].view.zero_()                          # (the one word the caller clears; a clean call must leave the sentinel alone)
    p = lambda x: None if x is None else x.data_ptr()
    out = lambda name: None if name in null else g[name].ptr()
    si = _ffi.SplSeqpackIn(n, inp.L_in, p(d["ids"]), p(d["lengths"]), p(d["off"]), p(d["lab"]), [p(b) for b in d["byt"]])
    o = _ffi.SplSeqpackOpts(inp.flags(keep_tail, mask_first), ref.STRATEGIES[strategy], L, 77, -100, FILLS)
    so = _ffi.SplSeqpackOut(R, g["rows"].ptr(), out("labels"), [out(f"b{k}") for k in range(4)], out("mask"), out("pos"), out("sid"),
                            out("place"), out("fill"), out("cu"), out("n"), g["status"].ptr())
    rc = lib.spl_seqpack_device(t.handle, ctypes.byref(si), ctypes.byref(o), ctypes.byref(so), g["work"].ptr(), _stream())
    assert rc == 0, _ffi.last_error()
    tag = (n, L, strategy, inp.form, inp.i64, inp.pad_left, keep_tail, max_rows, null)
    h = {k: v.host() for k, v in g.items()}              # (every guard is checked here)
    for k in null:
        assert (h[k] == g[k].sent).all(), (k,) + tag      # not wanted: not written
    a = {k: np.concatenate([v, v[:1]]) for k, v in h.items()}
    a["cu"] = np.where(a["cu"] == SENT["int32"], -1, a["cu"])
    assert h["status"].tolist() == [1 if want.status else SENT["int32"]], tag
    got = sim.to_packed(a, inp, n, R, L, want.status, null=null)
    if inp.lab is None and "labels" not in null:
        assert (h["labels"] == g["labels"].sent).all(), tag              # nothing to carry: not written
    for k in range(4):
        if inp.byt[k] is None and f"b{k}" not in null:
            assert (h[f"b{k}"] == g[f"b{k}"].sent).all(), tag
    try:
        sim.assert_equal(got, want)
    except AssertionError as e:
        raise AssertionError(tag) from e
    return got


def _variant(k):
    return dict(form=("rows", "csr")[k & 1], i64=bool(k & 2), pad_left=bool(k & 4)), bool(k & 8)


def _one(t, sim, lengths, L, strategy, k, *, max_rows=None, mask_first=True, null=(), companions=True):
    seqs, labels, byts = sim.content(lengths)
    kw, keep_tail = _variant(k)
    inp = sim.Inputs(seqs, labels=labels if companions else None, byte_arrays=byts if companions else (None,) * 4, **kw)
    want = ref.pack(seqs, L, strategy, max_rows=max_rows, pad_id=77, labels=labels if companions else None,
                    byte_arrays=byts if companions else (None,) * 4, fills=FILLS, keep_tail=keep_tail, mask_first=mask_first)
    got = _pack(t, sim, inp, _upload(inp), L, strategy, want, max_rows=max_rows, keep_tail=keep_tail, mask_first=mask_first, null=null)
    if not null:
        ref.check_invariants(got, lengths, L, len(lengths) if max_rows is None else max_rows)
    return got


# ------------------------------------------------------------------------------------------ 1. the grid
@pytest.mark.parametrize("L", [1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 130])
def test_seqpack_grid(sim, L):
    t = tok(NAME)
    cases = [c for c in sim.grid_cases() if c[2] == L]
    assert len(cases) == len(sim.N_SEQS)
    for k, (name, lengths, _) in enumerate(cases):
        rows = {s: int(_one(t, sim, lengths, L, s, k + 3 * i + L).n[0]) for i, s in enumerate(STRATEGIES)}
        assert rows["best_fit_decreasing"] <= rows["next_fit"], name


def test_seqpack_shaped_lengths_and_mask_first(sim):
    t = tok(NAME)
    for k, (name, lengths, L) in enumerate(sim.shaped_cases()):
        for s in STRATEGIES:
            _one(t, sim, lengths, L, s, k, mask_first=bool(k & 1))
    got = _one(t, sim, [4, 4, 3, 3, 3, 3], 7, "best_fit_decreasing", 0)
    assert got.seq_place.tolist() == [[0, 0], [1, 0], [1, 4], [0, 4], [2, 0], [2, 3]]           # the LIFO tie
    for mask_first in (True, False):
        got = _one(t, sim, [3, 2], 8, "next_fit", 2, mask_first=mask_first)
        assert (got.labels[0, 0] == -100) or not mask_first


def test_seqpack_thresholds_on_the_device(sim):
    """one below, at and one above the switch between the plans' LDS arrays and the work buffer -- lowered by "seqpack_lds_max" and at
    its default --, the plan workgroup's stride, and best_fit_decreasing's pool bound"""
    from splintr_amd import Tokenizer, _ffi
    lib = _ffi.lib()
    t = Tokenizer.from_pretrained(NAME)                   # (a handle of its own: the option is the handle's)
    g = sim.geometry()
    rng = np.random.default_rng(5)
    assert lib.spl_set_option(t.handle, b"seqpack_lds_max", g["lds_max"] + 1) == -1
    for lds_max in (0, 64):
        assert lib.spl_set_option(t.handle, b"seqpack_lds_max", lds_max) == 0
        for n in (63, 64, 65, 130):
            for s in STRATEGIES:
                _one(t, sim, rng.integers(0, 9, size=n).tolist(), 7, s, n)
    assert lib.spl_set_option(t.handle, b"seqpack_lds_max", g["lds_max"]) == 0
    for n in (g["plan_lanes"] - 1, g["plan_lanes"], g["plan_lanes"] + 1, g["lds_max"] - 1, g["lds_max"], g["lds_max"] + 1):
        for s in STRATEGIES:
            _one(t, sim, rng.integers(0, 19, size=n).tolist(), 16, s, 1, companions=False, max_rows=n // 4)
    L = g["bfd_max_l"]
    half = (g["pool"] - L - 1) // 2
    for n in (half - 1, half, half + 1):
        lengths = rng.integers(1, 64, size=n).tolist()
        lengths[0], lengths[5], lengths[n // 2] = L, L - 3, L // 2
        _one(t, sim, lengths, L, "best_fit_decreasing", 1, companions=False, max_rows=2,
             null=("labels", "b0", "b1", "b2", "b3", "pos", "sid"))


def test_seqpack_max_rows_and_optional_outputs(sim):
    t = tok(NAME)
    lengths = [5, 6, 7, 3, 9, 2, 8, 4, 1, 9, 9, 0, 12] * 5
    for s in STRATEGIES:
        need = len(ref.plan(lengths, 9, s).rows)
        for R in (0, 1, need - 1, need, need + 1):
            assert int(_one(t, sim, lengths, 9, s, R, max_rows=R).n[0]) == need
        for i, name in enumerate(sim.OUT_NAMES):
            _one(t, sim, lengths, 9, s, i, null=(name,))
        _one(t, sim, lengths, 9, s, 2, null=sim.OUT_NAMES)


def test_seqpack_status_for_bad_input(sim):
    t = tok(NAME)
    seqs, labels, byts = sim.content([4, 3, 5, 2, 6])
    for s in STRATEGIES:
        for over in ([4, -1, 5, 2, 6], [4, 3, 7, 2, 6]):
            bad = [i for i, (a, b) in enumerate(zip(over, [4, 3, 5, 2, 6])) if a != b]
            inp = sim.Inputs(seqs, "rows", L_in=6, labels=labels, lengths_override=over)
            _pack(t, sim, inp, _upload(inp), 8, s, ref.pack(seqs, 8, s, pad_id=77, labels=labels, bad=bad, fills=FILLS))
        off = [3, 7, 6, 11, 13, 19]
        inp = sim.Inputs(seqs, "csr", off_override=off)
        seqs2 = [inp.ids[off[i]:off[i + 1]].tolist() if off[i + 1] >= off[i] else [] for i in range(5)]
        _pack(t, sim, inp, _upload(inp), 8, s, ref.pack(seqs2, 8, s, pad_id=77, bad=[1], fills=FILLS))


# ------------------------------------------------------------------------------------------ 2. end to end
CONVS = [
    [("system", "You are a helpful assistant."), ("user", "What is 2 + 2?"), ("assistant", "4"), ("user", "And 3 + 3?"), ("assistant", "6 it is.\n")],
    [("system", "You are a helpful assistant."), ("user", "你好世界"), ("assistant", "Hello 🌍 World! ")],
    [("user", ""), ("assistant", "a"), ("user", "42 results\n\n"), ("assistant", "Done")],
    [("system", "You are a helpful assistant."), ("user", "naïve café?   ")],
    [],
    [("user", "Summarise: " + "the quick brown fox jumps over the lazy dog. " * 12), ("assistant", "A fox jumps over a dog.")],
    [("user", "hi"), ("assistant", "hello")],
]


def _template(t, name):
    from splintr_amd.chat import ChatTemplate
    return ChatTemplate.llama3(t) if name == "llama3" else ChatTemplate.chatml(t)


@pytest.mark.parametrize("name", ["llama3", "cl100k_base"])
def test_encode_batch_chat_packed_end_to_end(name):
    """encode_batch_chat_packed == chat_device followed by the reference's packing of its host copy, for every output; unpacking
    input_ids and labels by seq_place gives back chat_device's rows"""
    import torch
    t = tok(name)
    tpl = _template(t, name)
    convs = CONVS * 3
    L = 96
    for strategy, dtype, mask_first in (("best_fit_decreasing", torch.int32, True), ("next_fit", torch.int64, False)):
        chat = t.encode_batch_chat(convs, L, template=tpl, pad_id=0, dtype=dtype, check=True)
        lens = chat.lengths.cpu().numpy()
        rows, labels = chat.input_ids.cpu().numpy().astype(np.int64), chat.labels.cpu().numpy().astype(np.int64)
        byts = [x.cpu().numpy() for x in (chat.loss_mask, chat.role_ids, chat.special_tokens_mask)]
        cut = lambda a: [a[i, :lens[i]].tolist() for i in range(len(convs))]
        want = ref.pack(cut(rows), L, strategy, pad_id=0, labels=cut(labels), byte_arrays=tuple(cut(b) for b in byts) + (None,),
                        fills=(0, 255, 1, 0), mask_first=mask_first)
        out = t.encode_batch_chat_packed(convs, L, template=tpl, pad_id=0, strategy=strategy, dtype=dtype, mask_first=mask_first, trim=False)
        assert all(x is None or x.device.type == "cuda" for x in out) and out.input_ids.shape == (len(convs), L) and out.extra is None
        assert out.input_ids.dtype == out.labels.dtype == dtype
        host = lambda x: x.cpu().numpy()
        assert np.array_equal(host(out.input_ids), want.input_ids) and np.array_equal(host(out.labels), want.labels)
        for g, w in zip((out.loss_mask, out.role_ids, out.special_tokens_mask), want.bytes):
            assert np.array_equal(host(g), w)
        for g, w in ((out.attention_mask, want.attention_mask), (out.position_ids, want.position_ids), (out.seq_ids, want.seq_ids),
                     (out.seq_place, want.seq_place), (out.row_fill, want.row_fill), (out.n, want.n)):
            assert np.array_equal(host(g), w)
        k = int(want.n[2])
        assert np.array_equal(host(out.cu_seqlens)[:k], want.cu_seqlens[:k]) and int(out.status) == 0
        place, ids, lab = host(out.seq_place), host(out.input_ids), host(out.labels)
        for i in range(len(convs)):                      # unpacking gives chat_device's rows back
            r, c = place[i]
            if lens[i] == 0:
                assert (r, c) == (-1, -1)
                continue
            assert np.array_equal(ids[r, c:c + lens[i]], rows[i, :lens[i]])
            first = 1 if mask_first else 0
            assert np.array_equal(lab[r, c + first:c + lens[i]], labels[i, first:lens[i]]) and (not mask_first or lab[r, c] == -100)
        trimmed = t.encode_batch_chat_packed(convs, L, template=tpl, pad_id=0, strategy=strategy, dtype=dtype, mask_first=mask_first)
        n_rows = int(want.n[0])
        assert trimmed.input_ids.shape == (n_rows, L) and torch.equal(trimmed.input_ids, out.input_ids[:n_rows]) and \
            trimmed.cu_seqlens.shape == (k,) and int(trimmed.cu_seqlens[-1]) == n_rows * L and n_rows < len(convs)


@pytest.mark.parametrize("name", ["llama3", "cl100k_base"])
def test_encode_batch_packed_whole_end_to_end(coracle, name):
    """the oracle's per-document ids placed by the reference: the CSR form (no BOS / EOS) and the rows form (BOS and EOS), a document
    longer than the row cut at either end"""
    t, orc = tok(name), coracle(name)
    texts = ["Hello, world!", "", "你好世界", "naïve café " * 9, "a", "The quick brown fox jumps over the lazy dog. " * 5, "42", "Hello 🌍 World!"] * 4
    docs = orc.encode_batch(texts)
    L = 48
    for strategy, bos, eos, side in (("best_fit_decreasing", None, None, "right"), ("next_fit", None, None, "left"),
                                     ("best_fit_decreasing", 1, 2, "right"), ("next_fit", None, 2, "left")):
        k = (bos is not None) + (eos is not None)
        seqs = []
        for d in docs:
            body = d[:L - k] if side == "right" else d[max(0, len(d) - (L - k)):]
            seqs.append(([bos] if bos is not None else []) + body + ([eos] if eos is not None else []))
        want = ref.pack(seqs, L, strategy, pad_id=0)
        out = t.encode_batch_packed_whole(texts, L, pad_id=0, bos_id=bos, eos_id=eos, strategy=strategy, truncation_side=side)
        n_rows, kk = int(want.n[0]), int(want.n[2])
        host = lambda x: x.cpu().numpy()
        assert np.array_equal(host(out.input_ids), want.input_ids[:n_rows]) and out.labels is None and out.loss_mask is None
        assert np.array_equal(host(out.position_ids), want.position_ids[:n_rows]) and np.array_equal(host(out.seq_ids), want.seq_ids[:n_rows])
        assert np.array_equal(host(out.seq_place), want.seq_place) and np.array_equal(host(out.cu_seqlens), want.cu_seqlens[:kk])
        assert np.array_equal(host(out.attention_mask), want.attention_mask[:n_rows])
        n = host(out.n)
        assert n[0] == n_rows and n[1] == want.n[1] and (k or n[3] == sum(len(d) > L for d in docs))


def test_seqpack_on_a_side_stream(sim):
    """the call on a non-default stream, queued behind the upload with no synchronisation in between: the same outputs"""
    import torch
    from splintr_amd.device import seqpack_rows_device
    t = tok(NAME)
    lengths = np.random.default_rng(9).integers(0, 70, size=300).tolist()
    seqs, labels, byts = sim.content(lengths)
    inp = sim.Inputs(seqs, labels=labels)
    ids, lens, lab = (torch.from_numpy(a).to(_dev()) for a in (inp.ids, inp.lengths, inp.lab))
    want = seqpack_rows_device(t, ids, lens, 64, pad_id=0, labels=lab)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=_dev())
    with torch.cuda.stream(side):
        ids2, lens2, lab2 = ids.clone(), lens.clone(), lab.clone()
        out = seqpack_rows_device(t, ids2, lens2, 64, pad_id=0, labels=lab2)
    side.synchronize()
    k = int(want.n[2])
    for name, a, b in zip(out._fields, out, want):
        if a is None:
            assert b is None
        elif name == "cu_seqlens":
            assert torch.equal(a[:k], b[:k])
        else:
            assert torch.equal(a, b), name
    w = ref.pack(seqs, 64, "best_fit_decreasing", pad_id=0, labels=labels)
    assert np.array_equal(out.input_ids.cpu().numpy(), w.input_ids) and np.array_equal(out.labels.cpu().numpy(), w.labels)
