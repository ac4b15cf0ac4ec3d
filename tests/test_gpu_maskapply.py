"""GPU tests (-m gpu): spl_mask_apply_device -- an allowed-token bitmask applied to f32 / f16 / bf16 logits in place -- against numpy on the
bit patterns: every width around a 16-byte piece and a mask word, rows on odd boundaries, padded rows with canaries in the padding and
behind the last row, a sliced base, masks of all ones (the tensor unchanged bit for bit with NaN, +-inf and -0.0 planted), all zeros,
single bits at every position of two adjacent words and random ones, live bytes over poisoned mask rows; TokenHealer.apply against its
former torch-op composition; the refusals."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COLS = [1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 255, 257, 1000, 100336]
CANARY = {2: 0x5AC3, 4: 0x5AC3A53C}
NINF = {"float32": 0xFF800000, "float16": 0xFC00, "bfloat16": 0xFF80}
PLANT = {"float32": [0x7FC12345, 0xFFC00001, 0x7F800000, 0xFF800000, 0x80000000], "float16": [0x7E01, 0xFE02, 0x7C00, 0xFC00, 0x8000],
         "bfloat16": [0x7FC1, 0xFFC2, 0x7F80, 0xFF80, 0x8000]}


def _torch_dtype(name):
    import torch
    return getattr(torch, name)


def _uint(name):
    return np.uint32 if name == "float32" else np.uint16


def _patterns(rng, name, R, C):
    """bit patterns uint [R, C] with NaNs (payloads), +-inf and -0.0 planted"""
    es = 4 if name == "float32" else 2
    v = rng.integers(0, 1 << (8 * es), size=(R, C), dtype=np.uint64).astype(_uint(name))
    flat = v.reshape(-1)
    if flat.size:
        at = rng.integers(0, flat.size, size=min(flat.size, 5 * max(1, R)))
        flat[at] = np.resize(np.array(PLANT[name], dtype=_uint(name)), len(at))
    return v


def _expected(vals, name, mask, live, n_cols):
    R = vals.shape[0]
    want = vals.copy()
    n_eff = min(n_cols, 32 * mask.shape[1])
    if R and n_eff:
        bits = np.unpackbits(np.ascontiguousarray(mask).view(np.uint8).reshape(R, -1), axis=1, bitorder="little")[:, :n_eff].astype(bool)
        rows = np.ones(R, dtype=bool) if live is None else np.asarray(live).astype(bool)
        sub = want[:, :n_eff]
        sub[~bits & rows[:, None]] = NINF[name]
    return want


def _apply(tok, name, vals, mask, *, n_cols, base=0, live=None, mask_poison_rows=None, through="python"):
    """vals uint [R, stride]: the rows with their padding.  The logits live in a flat buffer with `base` elements in front and canaries
    behind; returns the rows afterwards.  Asserts that nothing in front of the first row or behind the last was written."""
    import torch
    from splintr_amd import device as dv
    dev = torch.device("cuda", 0)
    es = vals.dtype.itemsize
    R, stride = vals.shape
    int_t = torch.int32 if es == 4 else torch.int16
    flat = np.full(base + R * stride + 64, CANARY[es], dtype=vals.dtype)
    flat[base:base + R * stride] = vals.reshape(-1)
    buf = torch.from_numpy(flat.view(np.int32 if es == 4 else np.int16)).to(dev)
    logits = buf[base:base + R * stride].view(_torch_dtype(name)).reshape(R, stride)[:, :n_cols]
    t_mask = torch.from_numpy(np.ascontiguousarray(mask).view(np.int32)).to(dev)
    t_live = None if live is None else torch.from_numpy(np.ascontiguousarray(live, dtype=np.uint8)).to(dev)
    out = dv.mask_apply_device(tok, logits, t_mask, live=t_live)
    assert out is logits
    got = buf.cpu().numpy().view(vals.dtype)
    assert (got[:base] == CANARY[es]).all() and (got[base + R * stride:] == CANARY[es]).all(), "written in front of the rows or behind them"
    return got[base:base + R * stride].reshape(R, stride).copy()


@pytest.fixture(scope="module")
def tok():
    from splintr_amd import Tokenizer
    return Tokenizer.from_pretrained("cl100k_base")


def _masks(rng, R, n_words):
    return {"ones": np.full((R, n_words), 0xFFFFFFFF, dtype=np.uint32), "zeros": np.zeros((R, n_words), dtype=np.uint32),
            "random": rng.integers(0, 1 << 32, size=(R, n_words), dtype=np.uint64).astype(np.uint32),
            "sparse": (rng.integers(0, 1 << 32, size=(R, n_words), dtype=np.uint64) & rng.integers(0, 1 << 32, size=(R, n_words), dtype=np.uint64)
                       & rng.integers(0, 1 << 32, size=(R, n_words), dtype=np.uint64) & rng.integers(0, 1 << 32, size=(R, n_words), dtype=np.uint64)).astype(np.uint32)}


@pytest.mark.parametrize("name", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("n_cols", COLS)
def test_apply_against_numpy(tok, name, n_cols):
    rng = np.random.default_rng(n_cols)
    words = (n_cols + 31) // 32
    big = n_cols > 2000                                     # (the widest case: 257 rows once, every other combination at 0, 1 and 3 rows)
    combos = [(R, pad, base, n_words) for R in ((0, 1, 3) if big else (0, 1, 3, 257)) for pad, base in ((0, 0), (0, 1), (5, 1))
              for n_words in sorted({max(1, words - 1), words, words + 1})]
    if big:
        combos.append((257, 5, 1, words))
    for R, pad, base, n_words in combos:
        vals = _patterns(rng, name, R, n_cols + pad)
        for kind, mask in _masks(rng, R, n_words).items():
            if big and R == 257 and kind != "random":
                continue
            got = _apply(tok, name, vals, mask, n_cols=n_cols, base=base)
            assert (got == _expected(vals, name, mask, None, n_cols)).all(), (R, pad, base, n_words, kind)
            if kind == "ones":
                assert (got == vals).all()
            assert (got[:, n_cols:] == vals[:, n_cols:]).all()                  # the padding behind every row


@pytest.mark.parametrize("name", ["float32", "bfloat16"])
def test_single_bits_at_every_position_of_two_words(tok, name):
    rng = np.random.default_rng(2)
    n_cols, R = 101, 64
    vals = _patterns(rng, name, R, n_cols)
    for one in (False, True):
        mask = np.zeros((R, 4), dtype=np.uint32) if one else np.full((R, 4), 0xFFFFFFFF, dtype=np.uint32)
        for r in range(R):
            mask[r, 1 + r // 32] ^= np.uint32(1 << (r % 32))
        for base in (0, 1, 3):
            got = _apply(tok, name, vals, mask, n_cols=n_cols, base=base)
            assert (got == _expected(vals, name, mask, None, n_cols)).all(), (one, base)
            if not one:
                assert ((got != vals).sum(1) <= 1).all()


@pytest.mark.parametrize("name", ["float16", "float32"])
def test_live_rows_over_poisoned_mask_rows(tok, name):
    rng = np.random.default_rng(8)
    R, n_cols, n_words = 257, 333, 11
    vals = _patterns(rng, name, R, n_cols + 3)
    live = (rng.random(R) < 0.5).astype(np.uint8)
    mask = rng.integers(0, 1 << 32, size=(R, n_words), dtype=np.uint64).astype(np.uint32)
    poisoned = mask.copy()
    poisoned[live == 0] = 0                                                     # a row that is not live: all forbidden, if it were read
    got = _apply(tok, name, vals, poisoned, n_cols=n_cols, base=1, live=live)
    assert (got == _expected(vals, name, mask, live, n_cols)).all()
    assert (got[live == 0] == vals[live == 0]).all()
    got = _apply(tok, name, vals, poisoned, n_cols=n_cols, live=np.zeros(R, dtype=np.uint8))
    assert (got == vals).all()


def test_strided_mask_and_tokenizer_method(tok):
    import torch
    rng = np.random.default_rng(6)
    R, C, W = 5, 70, 3
    vals = _patterns(rng, "float32", R, C)
    wide = rng.integers(0, 1 << 32, size=(R, W + 2), dtype=np.uint64).astype(np.uint32)
    logits = torch.from_numpy(vals.view(np.int32)).cuda().view(torch.float32)
    t_mask = torch.from_numpy(wide.view(np.int32)).cuda()[:, :W]                # rows W + 2 words apart
    out = tok.apply_token_bitmask(logits, t_mask)
    assert out is logits
    assert (logits.view(torch.int32).cpu().numpy().view(np.uint32) == _expected(vals, "float32", wide[:, :W], None, C)).all()


def test_token_healer_apply_is_the_torch_composition(tok):
    """TokenHealer.apply through the kernel equals the torch ops it was made of, on the healer's masks of test_token_healer_end_to_end's
    prompts -- for the three dtypes, a width beyond the mask and one inside it, and live_only"""
    import torch
    texts = ["The link is http:", "def foo(", "Hello wor", "", "An answer with a trailing space ", "x = np.arr"]
    _, healer = tok.heal(texts, max_back=2)

    def former(logits):
        V = min(int(logits.shape[1]), 32 * healer.n_words)
        bits = ((healer.mask.unsqueeze(-1) >> torch.arange(32, device=healer.mask.device, dtype=torch.int32)) & 1).reshape(healer.batch_size, -1)
        logits[:, :V].masked_fill_(bits[:, :V] == 0, float("-inf"))
        return logits

    assert healer.live.any().item()
    torch.manual_seed(3)
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        for V in (tok.vocab_size + 5, tok.vocab_size - 1000, 32 * healer.n_words + 9):
            logits = torch.randn((len(texts), V), device=healer.mask.device).to(dtype)
            logits[1, 7] = float("nan")
            want = former(logits.clone())
            int_t = torch.int32 if dtype == torch.float32 else torch.int16
            for live_only in (False, True):
                got = healer.apply(logits.clone(), live_only=live_only)
                assert torch.equal(got.view(int_t), want.view(int_t)), (dtype, V, live_only)
    with pytest.raises(ValueError, match="shape"):
        healer.apply(torch.zeros((2, 8), device=healer.mask.device))


def test_refusals(tok):
    import torch
    from splintr_amd import _ffi, device as dv
    L = _ffi.lib()
    dev = torch.device("cuda", 0)
    logits = torch.zeros((2, 64), dtype=torch.float32, device=dev)
    mask = torch.full((2, 2), -1, dtype=torch.int32, device=dev)

    def go(word, h=tok.handle, **kw):
        f = dict(dtype=0, logits=logits.data_ptr(), n_rows=2, n_cols=64, n_words=2, row_stride=64, mask_stride=2, mask=mask.data_ptr(), live=None)
        f.update(kw)
        size = f.pop("struct_size", None)
        a = _ffi.SplMaskApply(**f)
        if size is not None:
            a.struct_size = size
        assert L.spl_mask_apply_device(h, ctypes.byref(a), None) == -1, word
        assert word in _ffi.last_error(), (word, _ffi.last_error())

    go("null handle", h=None)
    assert L.spl_mask_apply_device(tok.handle, None, None) == -1 and "request struct is null" in _ffi.last_error()
    go("struct_size", struct_size=8)
    go("dtype", dtype=3)
    go("d_logits is null", logits=None)
    go("d_mask is null", mask=None)
    go("row_stride is below n_cols", row_stride=63)
    go("mask_stride is below n_words", mask_stride=1)
    go("n_rows >= 2^31", n_rows=1 << 31)
    go("n_words is above 2^26", n_words=(1 << 26) + 1, mask_stride=(1 << 26) + 1)
    go("d_logits is not aligned", logits=logits.data_ptr() + 2)
    go("d_logits is not aligned", dtype=2, logits=logits.data_ptr() + 1)
    go("d_mask is not 4-byte aligned", mask=mask.data_ptr() + 2)
    a = _ffi.SplMaskApply(2, logits.data_ptr() + 2, 2, 60, 2, 64, 2, mask.data_ptr(), None)      # bf16 on an odd 2-byte boundary: fine
    assert L.spl_mask_apply_device(tok.handle, ctypes.byref(a), None) == 0
    torch.cuda.synchronize()
    # the Python layer: dtypes, shapes, layouts, devices
    for bad, word in (((logits.double(), mask), "float32, float16 or bfloat16"), ((logits[0], mask), "rank 2"), ((logits.t(), mask), "contiguous"),
                      ((logits, mask.long()), "int32 tensor"), ((logits, mask[:1]), "int32 tensor"), ((logits, mask.t()[:2]), "row of the mask"),
                      ((logits.cpu(), mask), "on a GPU"), ((logits, mask.cpu()), "device of the logits")):
        with pytest.raises(ValueError, match=word):
            dv.mask_apply_device(tok, *bad)
    with pytest.raises(ValueError, match="live"):
        dv.mask_apply_device(tok, logits, mask, live=torch.zeros(3, dtype=torch.uint8, device=dev))
    assert dv.mask_apply_device(tok, logits[:0], mask[:0]).shape == (0, 64)
