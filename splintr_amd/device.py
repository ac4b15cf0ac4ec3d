"""Device-resident batch encode: torch tensors in HBM in, CSR tensors in HBM out.

PyTorch is plumbing here (device memory, streams, torch.distributed); the work is done by
`spl_encode_batch_device` (include/splintr_hip.h) on torch's current HIP stream -- and, for a model on the same GPU, by
`spl_pad_device` / `spl_pack_device` behind it: the CSR as a padded batch or as packed sequences, one launch each.  The way back is
`spl_decode_batch_device`: ids in HBM (a CSR, or the rows a sampler leaves) to a bytes CSR in HBM.
"""
from __future__ import annotations

import ctypes
from collections import namedtuple
from collections.abc import Mapping
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _ffi
from .tokenizer import Tokenizer, _pack


def _raise_rc(rc: int, name: str):             # what the library refused (SPL_EINVAL) is a ValueError, anything else a RuntimeError
    raise (ValueError if rc == -1 else RuntimeError)(f"{name} failed ({rc}): {_ffi.last_error()}")


def _ptr(t):                                   # an optional tensor's address: null for None, True or an empty tensor
    return t.data_ptr() if isinstance(t, torch.Tensor) and t.numel() else None


def _vec(name: str, t, B: int, dtypes, what: str):            # (name, t) for a per-sequence argument of a batch of B
    if not isinstance(t, torch.Tensor) or t.dtype not in dtypes or t.dim() != 1 or t.shape[0] != B or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {what} tensor of shape [batch]")
    return name, t


class DeviceBatch:
    """A packed corpus resident on one GPU plus preallocated output buffers."""

    def __init__(self, texts: Sequence[str], device: torch.device):
        buf, off = _pack(texts)
        self.n_docs = len(off) - 1
        self.n_bytes = len(buf)
        pad = (-self.n_bytes) % 16 + 16
        host = np.frombuffer(buf + b"\0" * pad, dtype=np.uint8)
        self.text = torch.from_numpy(host.copy()).to(device)
        self.doc_off = torch.from_numpy(off.astype(np.int64)).to(device)
        self.ids = torch.empty(max(self.n_bytes, 1), dtype=torch.int32, device=device)
        self.out_off = torch.zeros(self.n_docs + 1, dtype=torch.int64, device=device)
        self.host_offsets = off


def encode_device(tok: Tokenizer, batch: DeviceBatch, with_special: bool = False) -> None:
    """One pass of the hot path over `batch`, asynchronous on torch's current stream.
    Results land in batch.ids / batch.out_off (out_off[-1] = token count)."""
    L = _ffi.lib()
    stream = torch.cuda.current_stream(batch.text.device).cuda_stream
    rc = L.spl_encode_batch_device(tok.handle, batch.text.data_ptr(), batch.n_bytes, batch.doc_off.data_ptr(),
                                   batch.n_docs, _ffi.SPL_WITH_SPECIAL if with_special else 0,
                                   batch.ids.data_ptr(), batch.ids.numel(), batch.out_off.data_ptr(), stream)
    if rc != 0:
        raise RuntimeError(f"spl_encode_batch_device failed ({rc}): {_ffi.last_error()}")


def reserve(tok: Tokenizer, n_bytes: int, n_docs: int) -> None:
    if _ffi.lib().spl_reserve(tok.handle, n_bytes, n_docs) != 0:
        raise RuntimeError(_ffi.last_error())


def result_csr(batch: DeviceBatch) -> Tuple[np.ndarray, np.ndarray]:
    off = batch.out_off.cpu().numpy().astype(np.uint64)
    ids = batch.ids[: int(off[-1])].cpu().numpy().view(np.uint32)
    return ids, off


def _collate_opts(row_len: int, pad_id: int, bos_id: Optional[int], eos_id: Optional[int], dtype, flags: int = 0):
    """spl_collate_opts for one call; ValueError for what the Python surface can refuse by itself."""
    if dtype not in (torch.int32, torch.int64):
        raise ValueError(f"dtype must be torch.int32 or torch.int64, not {dtype}")
    for name, v in (("pad_id", pad_id), ("bos_id", bos_id), ("eos_id", eos_id)):
        if v is not None and not 0 <= int(v) < (1 << 32):
            raise ValueError(f"{name} must fit 32 bits")
    if int(row_len) <= 0 or int(row_len) >= (1 << 32):
        raise ValueError("the row length must be in 1 .. 2**32 - 1")
    flags |= _ffi.SPL_COLLATE_I64 if dtype == torch.int64 else 0
    flags |= _ffi.SPL_COLLATE_BOS if bos_id is not None else 0
    flags |= _ffi.SPL_COLLATE_EOS if eos_id is not None else 0
    return _ffi.SplCollateOpts(flags, int(row_len), int(pad_id), int(bos_id or 0), int(eos_id or 0))


def _side(name: str, value: str) -> bool:
    if value not in ("right", "left"):
        raise ValueError(f"{name} must be 'right' or 'left', not {value!r}")
    return value == "left"


def check_collate_args(row_len: int, pad_id: int, bos_id: Optional[int], eos_id: Optional[int], dtype, padding_side: str = "right",
                       truncation_side: str = "right") -> None:
    """ValueError for a dtype, side string, id or row length that pad_device / pack_device would refuse -- for callers that want to
    know before they put a batch on the device."""
    _side("padding_side", padding_side)
    _side("truncation_side", truncation_side)
    _collate_opts(row_len, pad_id, bos_id, eos_id, dtype)


def pad_device(tok: Tokenizer, batch: DeviceBatch, max_length: int, *, pad_id: int, bos_id: Optional[int] = None,
               eos_id: Optional[int] = None, padding_side: str = "right", truncation_side: str = "right",
               dtype: torch.dtype = torch.int32) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """batch's CSR (encode_device) as a dense batch, ONE launch on torch's current stream (spl_pad_device): row d = [bos_id] + the ids
    of document d cut to max_length - (BOS + EOS) + [eos_id], padded with pad_id.  truncation_side "right" keeps a document's head,
    "left" its tail; BOS and EOS are never cut away.  Returns (input_ids [n_docs, L], attention_mask uint8 [n_docs, L], lengths int32
    [n_docs]); nothing synchronises."""
    flags = (_ffi.SPL_COLLATE_PAD_LEFT if _side("padding_side", padding_side) else 0) | \
        (_ffi.SPL_COLLATE_KEEP_TAIL if _side("truncation_side", truncation_side) else 0)
    o = _collate_opts(max_length, pad_id, bos_id, eos_id, dtype, flags)
    dev = batch.ids.device
    rows = torch.empty((batch.n_docs, o.row_len), dtype=dtype, device=dev)       # (every element is written by the kernel)
    mask = torch.empty((batch.n_docs, o.row_len), dtype=torch.uint8, device=dev)
    lens = torch.empty(batch.n_docs, dtype=torch.int32, device=dev)
    rc = _ffi.lib().spl_pad_device(tok.handle, batch.ids.data_ptr(), batch.out_off.data_ptr(), batch.n_docs, ctypes.byref(o),
                                   rows.data_ptr(), mask.data_ptr(), lens.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        _raise_rc(rc, "spl_pad_device")
    return rows, mask, lens


def pack_device(tok: Tokenizer, batch: DeviceBatch, seq_len: int, *, pad_id: int, bos_id: Optional[int] = None,
                eos_id: Optional[int] = None, dtype: torch.dtype = torch.int32,
                max_rows: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """batch's CSR as ONE stream -- [bos_id] ids_0 [eos_id] [bos_id] ids_1 [eos_id] ... -- cut into rows of seq_len, ONE launch on torch's
    current stream (spl_pack_device); nothing is truncated.  Returns (rows [max_rows, L], doc_ids int32 [max_rows, L], positions int32
    [max_rows, L], n): n is a DEVICE tensor (int64[2]: the rows the stream needs, its length), so nothing synchronises here; rows from
    n[0] on hold pad_id, doc_ids -1 there.  The default max_rows, ceil((batch.n_bytes + n_docs * (BOS + EOS)) / L), always suffices (a
    token has at least one byte); with a smaller one compare n[0] with it."""
    o = _collate_opts(seq_len, pad_id, bos_id, eos_id, dtype)
    k = (bos_id is not None) + (eos_id is not None)
    if max_rows is None:
        max_rows = (batch.n_bytes + batch.n_docs * k + o.row_len - 1) // o.row_len
    dev = batch.ids.device
    rows = torch.empty((int(max_rows), o.row_len), dtype=dtype, device=dev)      # (every element is written by the kernel)
    doc = torch.empty((int(max_rows), o.row_len), dtype=torch.int32, device=dev)
    pos = torch.empty((int(max_rows), o.row_len), dtype=torch.int32, device=dev)
    n = torch.empty(2, dtype=torch.int64, device=dev)
    rc = _ffi.lib().spl_pack_device(tok.handle, batch.ids.data_ptr(), batch.out_off.data_ptr(), batch.n_docs, ctypes.byref(o),
                                    rows.data_ptr(), int(max_rows), doc.data_ptr(), pos.data_ptr(), n.data_ptr(),
                                    torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        _raise_rc(rc, "spl_pack_device")
    return rows, doc, pos, n


def check_window_args(row_len: int, overlap: int, pad_id: int, bos_id: Optional[int], eos_id: Optional[int], dtype,
                      padding_side: str = "right") -> None:
    """check_collate_args for window_device: also ValueError for a row without room for a token beside BOS and EOS, and for an overlap
    outside 0 .. row_len - (BOS + EOS) - 1."""
    check_collate_args(row_len, pad_id, bos_id, eos_id, dtype, padding_side)
    budget = int(row_len) - (bos_id is not None) - (eos_id is not None)
    if budget < 1:
        raise ValueError("the row length must leave room for at least one token beside BOS and EOS")
    if isinstance(overlap, bool) or not isinstance(overlap, (int, np.integer)) or not 0 <= int(overlap) < budget:
        raise ValueError(f"overlap must be an integer in 0 .. {budget - 1} (the row length minus BOS, EOS and one), not {overlap!r}")


def window_device(tok: Tokenizer, batch: DeviceBatch, max_length: int, *, overlap: int = 0, pad_id: int, bos_id: Optional[int] = None,
                  eos_id: Optional[int] = None, padding_side: str = "right", dtype: torch.dtype = torch.int32,
                  max_rows: Optional[int] = None):
    """batch's CSR as SLIDING WINDOWS on torch's current stream (spl_window_device): every document alone and complete, as rows of
    max_length whose bodies (max_length - (BOS + EOS) ids) overlap by `overlap` ids -- Hugging Face's return_overflowing_tokens with
    stride = overlap.  Nothing is truncated and no row holds two documents; only a document's last window can be short.  Returns (rows
    [max_rows, L], mask uint8 [max_rows, L], lengths int32 [max_rows], row_doc int32 [max_rows], row_start int64 [max_rows], row_off int64
    [n_docs + 1], n): row r is window r - row_off[row_doc[r]] of document row_doc[r] and starts at id row_start[r] of it; n is a DEVICE
    tensor (int64[2]: the rows needed, the rows of these that fit max_rows), so nothing synchronises here; rows from n[0] on hold pad_id,
    row_doc -1.  The default max_rows, n_docs + batch.n_bytes // step with step = max_length - (BOS + EOS) - overlap, always suffices: a
    document of len ids needs one row, or beyond the body budget B 1 + ceil((len - B) / step) <= 1 + (len - 1) // step of them (because
    B >= step), so all documents together at most n_docs + (all ids) // step, and a token has at least one byte; with a smaller one
    compare n[0] with it."""
    check_window_args(max_length, overlap, pad_id, bos_id, eos_id, dtype, padding_side)
    o = _collate_opts(max_length, pad_id, bos_id, eos_id, dtype, _ffi.SPL_COLLATE_PAD_LEFT if _side("padding_side", padding_side) else 0)
    step = o.row_len - (bos_id is not None) - (eos_id is not None) - int(overlap)
    if max_rows is None:
        max_rows = batch.n_docs + batch.n_bytes // step
    max_rows = int(max_rows)
    dev = batch.ids.device
    L = _ffi.lib()
    rows = torch.empty((max_rows, o.row_len), dtype=dtype, device=dev)           # (every element is written by the kernel)
    mask = torch.empty((max_rows, o.row_len), dtype=torch.uint8, device=dev)
    lens = torch.empty(max_rows, dtype=torch.int32, device=dev)
    row_doc = torch.empty(max_rows, dtype=torch.int32, device=dev)
    row_start = torch.empty(max_rows, dtype=torch.int64, device=dev)
    row_off = torch.empty(batch.n_docs + 1, dtype=torch.int64, device=dev)
    n = torch.empty(2, dtype=torch.int64, device=dev)
    work = torch.empty(int(L.spl_window_work_bytes(batch.n_docs)), dtype=torch.uint8, device=dev)
    rc = L.spl_window_device(tok.handle, batch.ids.data_ptr(), batch.out_off.data_ptr(), batch.n_docs, ctypes.byref(o), int(overlap),
                             rows.data_ptr() if max_rows else None, max_rows, mask.data_ptr() if max_rows else None,
                             lens.data_ptr() if max_rows else None, row_doc.data_ptr() if max_rows else None,
                             row_start.data_ptr() if max_rows else None, row_off.data_ptr(), n.data_ptr(),
                             work.data_ptr() if work.numel() else None, torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        _raise_rc(rc, "spl_window_device")
    return rows, mask, lens, row_doc, row_start, row_off, n


# ---------------------------------------------------------------------------------------------- pairs: two CSRs, one row per pair
_TRUNCATION = {"longest_first": _ffi.SPL_PAIR_LONGEST_FIRST, "only_first": _ffi.SPL_PAIR_ONLY_FIRST, "only_second": _ffi.SPL_PAIR_ONLY_SECOND}


def _segment(name: str, ids) -> Tuple[int, ...]:
    if isinstance(ids, (str, bytes)) or not isinstance(ids, (list, tuple)):
        raise ValueError(f"{name} must be a list or tuple of ids, not {type(ids).__name__}")
    if len(ids) > _ffi.SPL_PAIR_MAX_FIXED:
        raise ValueError(f"{name} holds {len(ids)} ids: a fixed segment holds at most {_ffi.SPL_PAIR_MAX_FIXED}")
    for v in ids:
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < (1 << 32):
            raise ValueError(f"every id of {name} must be an integer that fits 32 bits, not {v!r}")
    return tuple(int(v) for v in ids)


def _pair_opts(row_len: int, pad_id: int, prefix, middle, suffix, truncation: str, truncation_side_a: str, truncation_side_b: str,
               padding_side: str, dtype):
    """spl_pair_opts for one call; ValueError for what the Python surface can refuse by itself."""
    if dtype not in (torch.int32, torch.int64):
        raise ValueError(f"dtype must be torch.int32 or torch.int64, not {dtype}")
    if truncation not in _TRUNCATION:
        raise ValueError(f"truncation must be 'longest_first', 'only_first' or 'only_second', not {truncation!r}")
    flags = (_ffi.SPL_COLLATE_I64 if dtype == torch.int64 else 0) | \
        (_ffi.SPL_COLLATE_PAD_LEFT if _side("padding_side", padding_side) else 0) | \
        (_ffi.SPL_PAIR_KEEP_TAIL_A if _side("truncation_side_a", truncation_side_a) else 0) | \
        (_ffi.SPL_PAIR_KEEP_TAIL_B if _side("truncation_side_b", truncation_side_b) else 0)
    if isinstance(pad_id, bool) or not isinstance(pad_id, (int, np.integer)) or not 0 <= int(pad_id) < (1 << 32):
        raise ValueError("pad_id must fit 32 bits")
    segs = [_segment(n, v) for n, v in (("prefix", prefix), ("middle", middle), ("suffix", suffix))]
    if isinstance(row_len, bool) or not isinstance(row_len, (int, np.integer)) or int(row_len) <= 0 or int(row_len) >= (1 << 32):
        raise ValueError("the row length must be in 1 .. 2**32 - 1")
    if int(row_len) < sum(map(len, segs)):
        raise ValueError(f"the row length {int(row_len)} is smaller than the {sum(map(len, segs))} ids of prefix + middle + suffix every row holds")
    return _ffi.SplPairOpts(flags, int(row_len), int(pad_id), _TRUNCATION[truncation], *segs)


def check_pair_args(row_len: int, pad_id: int, prefix=(), middle=(), suffix=(), truncation: str = "longest_first",
                    truncation_side_a: str = "right", truncation_side_b: str = "right", padding_side: str = "right",
                    dtype=torch.int32) -> None:
    """ValueError for a dtype, truncation or side string, id, fixed segment or row length that pair_device would refuse -- for callers
    that want to know before they put a batch on the device."""
    _pair_opts(row_len, pad_id, prefix, middle, suffix, truncation, truncation_side_a, truncation_side_b, padding_side, dtype)


def _pair_index(name: str, index, dev) -> Optional[torch.Tensor]:
    if index is None:
        return None
    if not isinstance(index, torch.Tensor):
        index = torch.as_tensor(np.asarray(index, dtype=np.int64).astype(np.int32), device=dev)
    if index.dtype != torch.int32 or index.dim() != 1 or not index.is_contiguous() or index.device != dev:
        raise ValueError(f"{name} must be a contiguous int32 tensor of rank 1 on the device of the ids (or a sequence of integers)")
    return index


def pair_csr_device(tok: Tokenizer, a_ids: torch.Tensor, a_off: torch.Tensor, n_a: int, b_ids: torch.Tensor, b_off: torch.Tensor,
                    n_b: int, max_length: int, *, pad_id: int, prefix=(), middle=(), suffix=(), a_index=None, b_index=None,
                    truncation: str = "longest_first", truncation_side_a: str = "right", truncation_side_b: str = "right",
                    padding_side: str = "right", dtype: torch.dtype = torch.int32):
    """pair_device's low-level form: each side is (ids int32 [capacity], offsets int64 [at least n + 1], n documents), the offsets
    ABSOLUTE into ids and offsets[0] any value -- so the two sides may be two slices of ONE encode result: a = (ids, out_off, n_a),
    b = (ids, out_off[n_a:], n_b).  Same return as pair_device."""
    o = _pair_opts(max_length, pad_id, prefix, middle, suffix, truncation, truncation_side_a, truncation_side_b, padding_side, dtype)
    n_a, n_b = int(n_a), int(n_b)
    for name, ids, off, n in (("a", a_ids, a_off, n_a), ("b", b_ids, b_off, n_b)):
        if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int32 or ids.dim() != 1 or not ids.is_contiguous():
            raise ValueError(f"{name}_ids must be a contiguous int32 tensor of rank 1")
        if not isinstance(off, torch.Tensor) or off.dtype != torch.int64 or off.dim() != 1 or not off.is_contiguous() or \
                n < 0 or off.shape[0] < n + 1:
            raise ValueError(f"{name}_off must be a contiguous int64 tensor of at least n_{name} + 1 entries")
        if not ids.is_cuda or off.device != ids.device:
            raise ValueError(f"{name}_ids and {name}_off must be on one GPU")
    dev = a_ids.device
    if b_ids.device != dev:
        raise ValueError("the two sides must be on one GPU")
    a_index, b_index = _pair_index("a_index", a_index, dev), _pair_index("b_index", b_index, dev)
    if a_index is not None and b_index is not None and a_index.shape[0] != b_index.shape[0]:
        raise ValueError(f"a_index names {a_index.shape[0]} pairs, b_index {b_index.shape[0]}")
    if a_index is None and b_index is None and n_a != n_b:
        raise ValueError(f"without an index pair i is (a_i, b_i): the sides must hold equally many documents, not {n_a} and {n_b}")
    n_pairs = int(a_index.shape[0]) if a_index is not None else int(b_index.shape[0]) if b_index is not None else n_a
    if (a_index is None and n_pairs > n_a) or (b_index is None and n_pairs > n_b):
        raise ValueError(f"{n_pairs} pairs, but the side without an index holds fewer documents")
    new = lambda *shape, dt: torch.empty(*shape, dtype=dt, device=dev)          # (every element is written by the kernel)
    rows = new(n_pairs, o.row_len, dt=dtype)
    mask, ttype, special = (new(n_pairs, o.row_len, dt=torch.uint8) for _ in range(3))
    lens, kept = new(n_pairs, dt=torch.int32), new(n_pairs, 2, dt=torch.int32)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    # (d_rows may never be null; without a pair nothing is written, and an empty tensor has no address: any aligned one stands in)
    rc = _ffi.lib().spl_pair_device(tok.handle, a_ids.data_ptr(), a_off.data_ptr(), n_a, b_ids.data_ptr(), b_off.data_ptr(), n_b,
                                    _ptr(a_index), _ptr(b_index), n_pairs, ctypes.byref(o), rows.data_ptr() if n_pairs else status.data_ptr(),
                                    _ptr(mask), _ptr(ttype), _ptr(special), _ptr(lens), _ptr(kept), status.data_ptr(),
                                    torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        _raise_rc(rc, "spl_pair_device")
    return rows, mask, ttype, special, lens, kept, status


def pair_device(tok: Tokenizer, batch_a: DeviceBatch, batch_b: DeviceBatch, max_length: int, *, pad_id: int, prefix=(), middle=(),
                suffix=(), a_index=None, b_index=None, truncation: str = "longest_first", truncation_side_a: str = "right",
                truncation_side_b: str = "right", padding_side: str = "right", dtype: torch.dtype = torch.int32):
    """Two CSRs (encode_device on each batch; batch_b may be batch_a itself) as ONE ROW PER PAIR, one launch on torch's current stream
    (spl_pair_device): row p = prefix + A' + middle + B' + suffix padded with pad_id, where A' / B' are document a_index[p] of batch_a
    and b_index[p] of batch_b (int32 device tensors or sequences; None: document p) cut to max_length - len(prefix + middle + suffix)
    ids together -- "longest_first" (Hugging Face's rule: one id at a time from the longer side, from B on a tie), "only_first" or
    "only_second"; truncation_side_a / _b "right" keeps that side's head, "left" its tail.  The fixed segments are never cut away:
    BERT's [CLS] a [SEP] b [SEP] is prefix=[cls], middle=[sep], suffix=[sep].  Returns (input_ids [n_pairs, L], attention_mask uint8,
    token_type_ids uint8 (0 over prefix + A' + middle, 1 over B' + suffix, 0 on padding), special_tokens_mask uint8 (1 on the fixed
    segments and on padding), lengths int32 [n_pairs], kept int32 [n_pairs, 2] (the ids of each side that are in the row), status int32
    [1] (1: an index named no document -- that side of the pair is empty)); all device tensors, nothing synchronises."""
    return pair_csr_device(tok, batch_a.ids, batch_a.out_off, batch_a.n_docs, batch_b.ids, batch_b.out_off, batch_b.n_docs, max_length,
                           pad_id=pad_id, prefix=prefix, middle=middle, suffix=suffix, a_index=a_index, b_index=b_index,
                           truncation=truncation, truncation_side_a=truncation_side_a, truncation_side_b=truncation_side_b,
                           padding_side=padding_side, dtype=dtype)


# ---------------------------------------------------------------------------------------------- chat: a CSR of messages, one row per conversation
ChatRows = namedtuple("ChatRows", "input_ids labels attention_mask role_ids loss_mask special_tokens_mask lengths kept turn_cols status")


def _chat_opts(row_len: int, pad_id: int, template, add_generation_prompt: bool, truncation: str, pin_system: bool, padding_side: str,
               ignore_index: int, dtype):
    """spl_chat_opts for one call; ValueError for what the Python surface can refuse by itself."""
    from .chat import ChatTemplate
    if not isinstance(template, ChatTemplate):
        raise ValueError(f"template must be a splintr_amd.chat.ChatTemplate, not {type(template).__name__}")
    if dtype not in (torch.int32, torch.int64):
        raise ValueError(f"dtype must be torch.int32 or torch.int64, not {dtype}")
    if truncation not in ("right", "drop_oldest"):
        raise ValueError(f"truncation must be 'right' or 'drop_oldest', not {truncation!r}")
    if pin_system and truncation != "drop_oldest":
        raise ValueError("pin_system keeps the first turn while older ones are dropped: it needs truncation='drop_oldest'")
    flags = (_ffi.SPL_COLLATE_I64 if dtype == torch.int64 else 0) | \
        (_ffi.SPL_COLLATE_PAD_LEFT if _side("padding_side", padding_side) else 0) | \
        (_ffi.SPL_CHAT_DROP_OLDEST if truncation == "drop_oldest" else 0) | (_ffi.SPL_CHAT_PIN_FIRST if pin_system else 0)
    if isinstance(pad_id, bool) or not isinstance(pad_id, (int, np.integer)) or not 0 <= int(pad_id) < (1 << 32):
        raise ValueError("pad_id must fit 32 bits")
    if isinstance(ignore_index, bool) or not isinstance(ignore_index, (int, np.integer)) or not -(1 << 31) <= int(ignore_index) < (1 << 32):
        raise ValueError("ignore_index must fit 32 bits (a negative one is sign-extended in int64 labels)")
    gen = template.generation if add_generation_prompt else ()
    if isinstance(row_len, bool) or not isinstance(row_len, (int, np.integer)) or int(row_len) <= 0 or int(row_len) >= (1 << 32):
        raise ValueError("the row length must be in 1 .. 2**32 - 1")
    if int(row_len) < len(template.bos) + len(gen):
        raise ValueError(f"the row length {int(row_len)} is smaller than the {len(template.bos) + len(gen)} ids of bos + generation prompt every row holds")
    return _ffi.SplChatOpts(flags, int(row_len), int(pad_id), int(ignore_index) & 0xFFFFFFFF, list(template.roles.values()),
                            template.train_content_mask, template.train_footer_mask, template.bos, gen)


def check_chat_args(row_len: int, pad_id: int, template, add_generation_prompt: bool = False, truncation: str = "right",
                    pin_system: bool = False, padding_side: str = "right", ignore_index: int = -100, dtype=torch.int32) -> None:
    """ValueError for a template, dtype, truncation or side string, id or row length that chat_device would refuse -- for callers that
    want to know before they put a batch on the device."""
    _chat_opts(row_len, pad_id, template, add_generation_prompt, truncation, pin_system, padding_side, ignore_index, dtype)


def chat_turns(conversations, template, train_turns=None):
    """Conversations (sequences of {"role", "content"} dicts or (role, content) tuples) as host arrays: (texts, turn_doc int32, turn_role
    uint8, turn_train uint8 or None, conv_off int64).  EQUAL content strings are one text: a system prompt that ten thousand conversations
    share is encoded once.  train_turns: None, or per conversation a sequence of truth values, one per turn (False: the turn carries no
    labels whatever its role).  ValueError for a malformed message or a role the template does not have."""
    from .chat import message
    if isinstance(conversations, (str, bytes, Mapping)) or not hasattr(conversations, "__len__"):
        raise ValueError(f"conversations must be a sequence of conversations, not {type(conversations).__name__}")
    if train_turns is not None and len(train_turns) != len(conversations):
        raise ValueError("train_turns must hold one sequence per conversation")
    texts, index, turn_doc, turn_role, turn_train, conv_off = [], {}, [], [], [], [0]
    for c, conv in enumerate(conversations):
        if isinstance(conv, (str, bytes, Mapping)) or not hasattr(conv, "__len__"):
            raise ValueError(f"conversation {c} must be a sequence of messages, not {type(conv).__name__}")
        if train_turns is not None and len(train_turns[c]) != len(conv):
            raise ValueError(f"train_turns[{c}] must hold one value per turn of conversation {c}")
        for i, m in enumerate(conv):
            role, content = message(m)
            turn_role.append(template.role_of(role))
            if content not in index:
                index[content] = len(texts)
                texts.append(content)
            turn_doc.append(index[content])
            turn_train.append(1 if train_turns is None or train_turns[c][i] else 0)
        conv_off.append(len(turn_doc))
    if len(turn_doc) >= (1 << 31) or len(conv_off) > (1 << 31):
        raise ValueError("fewer than 2**31 turns and conversations")
    return (texts, np.array(turn_doc, dtype=np.int32), np.array(turn_role, dtype=np.uint8),
            None if train_turns is None else np.array(turn_train, dtype=np.uint8), np.array(conv_off, dtype=np.int64))


def chat_csr_device(tok: Tokenizer, ids: torch.Tensor, off: torch.Tensor, n_docs: int, turn_doc: Optional[torch.Tensor],
                    turn_role: torch.Tensor, conv_off: torch.Tensor, max_length: int, *, template, pad_id: int,
                    add_generation_prompt: bool = False, truncation: str = "right", pin_system: bool = False, padding_side: str = "right",
                    ignore_index: int = -100, turn_train: Optional[torch.Tensor] = None, dtype: torch.dtype = torch.int32) -> ChatRows:
    """chat_device's low-level form: the messages are (ids int32 [capacity], offsets int64 [at least n_docs + 1], ABSOLUTE into ids),
    turn t has the role number turn_role[t] (uint8 [n_turns]; template.role_of) and the content document turn_doc[t] (int32; None: t),
    conversation c owns the turns conv_off[c] .. conv_off[c + 1] - 1 (int64 [n_convs + 1]); turn_train (uint8, optional): 0 takes a
    turn's labels away.  Same return as chat_device."""
    o = _chat_opts(max_length, pad_id, template, add_generation_prompt, truncation, pin_system, padding_side, ignore_index, dtype)
    n_docs = int(n_docs)
    if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int32 or ids.dim() != 1 or not ids.is_contiguous() or not ids.is_cuda:
        raise ValueError("ids must be a contiguous int32 tensor of rank 1 on a GPU")
    dev = ids.device
    if not isinstance(off, torch.Tensor) or off.dtype != torch.int64 or off.dim() != 1 or not off.is_contiguous() or n_docs < 0 or \
            off.shape[0] < n_docs + 1 or off.device != dev:
        raise ValueError("off must be a contiguous int64 tensor of at least n_docs + 1 entries on the device of the ids")
    if not isinstance(turn_role, torch.Tensor) or turn_role.dtype != torch.uint8 or turn_role.dim() != 1 or not turn_role.is_contiguous() or \
            turn_role.device != dev:
        raise ValueError("turn_role must be a contiguous uint8 tensor of rank 1 on the device of the ids")
    n_turns = int(turn_role.shape[0])
    for name, t, dt in (("turn_doc", turn_doc, torch.int32), ("turn_train", turn_train, torch.uint8)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != 1 or t.shape[0] != n_turns or
                              not t.is_contiguous() or t.device != dev):
            raise ValueError(f"{name} must be a contiguous {str(dt).split('.')[-1]} tensor of shape [n_turns] on the device of the ids")
    if turn_doc is None and n_turns > n_docs:
        raise ValueError(f"without turn_doc turn t reads document t: {n_turns} turns need as many documents, not {n_docs}")
    if not isinstance(conv_off, torch.Tensor) or conv_off.dtype != torch.int64 or conv_off.dim() != 1 or conv_off.shape[0] < 1 or \
            not conv_off.is_contiguous() or conv_off.device != dev:
        raise ValueError("conv_off must be a contiguous int64 tensor of shape [n_convs + 1] on the device of the ids")
    n_convs = int(conv_off.shape[0]) - 1
    L = _ffi.lib()
    new = lambda *shape, dt: torch.empty(*shape, dtype=dt, device=dev)          # (every element is written by the kernels)
    rows, labels = new(n_convs, o.row_len, dt=dtype), new(n_convs, o.row_len, dt=dtype)
    mask, role, loss, special = (new(n_convs, o.row_len, dt=torch.uint8) for _ in range(4))
    lens, kept = new(n_convs, dt=torch.int32), new(n_convs, 2, dt=torch.int32)
    turn_cols = torch.full((n_turns, 2), -1, dtype=torch.int32, device=dev)     # (a turn outside every conversation is not written)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    work = torch.empty(int(L.spl_chat_work_bytes(n_turns, n_convs)), dtype=torch.uint8, device=dev)
    # (d_rows may never be null; without a conversation nothing is written, and an empty tensor has no address: any aligned one stands in)
    rc = L.spl_chat_device(tok.handle, ids.data_ptr(), off.data_ptr(), n_docs, _ptr(turn_doc), turn_role.data_ptr() if n_turns else None,
                           _ptr(turn_train), n_turns, conv_off.data_ptr(), n_convs, ctypes.byref(o),
                           rows.data_ptr() if n_convs else work.data_ptr(), _ptr(labels), _ptr(loss), _ptr(mask), _ptr(role), _ptr(special),
                           _ptr(lens), _ptr(kept), _ptr(turn_cols), status.data_ptr(), work.data_ptr(),
                           torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        _raise_rc(rc, "spl_chat_device")
    return ChatRows(rows, labels, mask, role, loss, special, lens, kept, turn_cols, status)


def chat_device(tok: Tokenizer, batch: DeviceBatch, turn_doc: Optional[torch.Tensor], turn_role: torch.Tensor, conv_off: torch.Tensor,
                max_length: int, *, template, pad_id: int, add_generation_prompt: bool = False, truncation: str = "right",
                pin_system: bool = False, padding_side: str = "right", ignore_index: int = -100,
                turn_train: Optional[torch.Tensor] = None, dtype: torch.dtype = torch.int32) -> ChatRows:
    """batch's CSR (encode_device: one document per distinct MESSAGE) as ONE ROW PER CONVERSATION with labels, two launches on torch's
    current stream (spl_chat_device): row c = bos + the turns of conversation c, each as its role's header + the message's ids + its
    role's footer, + the generation prompt (add_generation_prompt), padded with pad_id.  A body longer than max_length - len(bos +
    generation prompt) is cut on the right (truncation "right") or loses whole turns from the front until it fits ("drop_oldest";
    pin_system keeps turn 0); bos and the generation prompt are never cut away.  The control tokens come from `template`
    (splintr_amd.chat.ChatTemplate), never from message text.  Returns ChatRows: input_ids [n_convs, L]; labels (same dtype: the id on
    content and footer of the turns whose role the template trains -- and whose turn_train is not 0 --, ignore_index elsewhere, not
    shifted); attention_mask uint8; role_ids uint8 (the role number over a turn's header, content and footer, 255 elsewhere);
    loss_mask uint8 (1 where labels hold an id); special_tokens_mask uint8 (1 on template ids and padding); lengths int32 [n_convs];
    kept int32 [n_convs, 2] (turns dropped, body entries cut off on the right); turn_cols int32 [n_turns, 2] (the columns of turn t's
    content in its row, (-1, -1) if it is not there); status int32 [1] (1: a role, document index or turn range was out of range).
    All device tensors, nothing synchronises."""
    return chat_csr_device(tok, batch.ids, batch.out_off, batch.n_docs, turn_doc, turn_role, conv_off, max_length, template=template,
                           pad_id=pad_id, add_generation_prompt=add_generation_prompt, truncation=truncation, pin_system=pin_system,
                           padding_side=padding_side, ignore_index=ignore_index, turn_train=turn_train, dtype=dtype)


# ---------------------------------------------------------------------------------------------- whole-sequence packing
PackedRows = namedtuple("PackedRows", "input_ids labels attention_mask position_ids seq_ids loss_mask role_ids special_tokens_mask extra "
                                      "seq_place row_fill cu_seqlens n status")
SEQPACK_STRATEGIES = {"next_fit": _ffi.SPL_SEQPACK_NEXT_FIT, "best_fit_decreasing": _ffi.SPL_SEQPACK_BEST_FIT_DECREASING}
SEQPACK_FILLS = (0, _ffi.SPL_CHAT_NO_ROLE, 1, 0)     # what pads loss_mask, role_ids, special_tokens_mask, extra: chat_device's own padding


def _seqpack_opts(row_len: int, pad_id: int, strategy: str, ignore_index: int, fills, truncation_side: str, padding_side: str,
                  mask_first: bool, dtype, max_rows):
    """spl_seqpack_opts for one call; ValueError for what the Python surface can refuse by itself."""
    if strategy not in SEQPACK_STRATEGIES:
        raise ValueError(f"strategy must be 'next_fit' or 'best_fit_decreasing', not {strategy!r}")
    if dtype not in (torch.int32, torch.int64):
        raise ValueError(f"dtype must be torch.int32 or torch.int64, not {dtype}")
    if isinstance(pad_id, bool) or not isinstance(pad_id, (int, np.integer)) or not 0 <= int(pad_id) < (1 << 32):
        raise ValueError("pad_id must fit 32 bits")
    if isinstance(ignore_index, bool) or not isinstance(ignore_index, (int, np.integer)) or not -(1 << 31) <= int(ignore_index) < (1 << 32):
        raise ValueError("ignore_index must fit 32 bits (a negative one is sign-extended in int64 labels)")
    if isinstance(row_len, bool) or not isinstance(row_len, (int, np.integer)) or int(row_len) <= 0 or int(row_len) >= (1 << 32):
        raise ValueError("the row length must be in 1 .. 2**32 - 1")
    if strategy == "best_fit_decreasing" and int(row_len) > _ffi.SPL_SEQPACK_BFD_MAX_ROW_LEN:
        raise ValueError(f"best_fit_decreasing takes rows of up to {_ffi.SPL_SEQPACK_BFD_MAX_ROW_LEN} ids; next_fit has no such bound")
    fills = tuple(fills)
    if len(fills) != 4 or any(isinstance(f, bool) or not isinstance(f, (int, np.integer)) or not 0 <= int(f) < 256 for f in fills):
        raise ValueError("fills must be four byte values: what pads loss_mask, role_ids, special_tokens_mask and extra")
    if max_rows is not None and (isinstance(max_rows, bool) or not isinstance(max_rows, (int, np.integer)) or not 0 <= int(max_rows) < (1 << 31)):
        raise ValueError("max_rows must be in 0 .. 2**31 - 1")
    flags = (_ffi.SPL_COLLATE_I64 if dtype == torch.int64 else 0) | \
        (_ffi.SPL_COLLATE_PAD_LEFT if _side("padding_side", padding_side) else 0) | \
        (_ffi.SPL_COLLATE_KEEP_TAIL if _side("truncation_side", truncation_side) else 0) | (_ffi.SPL_SEQPACK_MASK_FIRST if mask_first else 0)
    return _ffi.SplSeqpackOpts(flags, SEQPACK_STRATEGIES[strategy], int(row_len), int(pad_id), int(ignore_index) & 0xFFFFFFFF, fills)


def check_seqpack_args(row_len: int, *, pad_id: int, strategy: str = "best_fit_decreasing", ignore_index: int = -100, fills=SEQPACK_FILLS,
                       truncation_side: str = "right", padding_side: str = "right", mask_first: bool = True, dtype=torch.int32,
                       max_rows: Optional[int] = None) -> None:
    """ValueError for a strategy, dtype, side string, id, fill, row length or max_rows that seqpack_rows_device / seqpack_csr_device would
    refuse -- for callers that want to know before they put a batch on the device."""
    _seqpack_opts(row_len, pad_id, strategy, ignore_index, fills, truncation_side, padding_side, mask_first, dtype, max_rows)


def _seqpack_call(tok: Tokenizer, o, si, dev, n_seqs: int, have_labels: bool, have_bytes, dtype, max_rows: Optional[int]) -> PackedRows:
    R = n_seqs if max_rows is None else int(max_rows)
    L, row_len = _ffi.lib(), o.row_len
    if R * row_len >= (1 << 31):
        raise ValueError(f"cu_seqlens is int32: max_rows * seq_len = {R * row_len} must be below 2**31")
    new = lambda *shape, dt: torch.empty(*shape, dtype=dt, device=dev)          # (every element is written by the kernels)
    rows = new(R, row_len, dt=dtype)
    labels = new(R, row_len, dt=dtype) if have_labels else None
    byts = [new(R, row_len, dt=torch.uint8) if h else None for h in have_bytes]
    mask, pos, seq = new(R, row_len, dt=torch.uint8), new(R, row_len, dt=torch.int32), new(R, row_len, dt=torch.int32)
    place, fill, n = new(n_seqs, 2, dt=torch.int32), new(R, dt=torch.int32), new(4, dt=torch.int64)
    cu = torch.zeros(n_seqs + R + 1, dtype=torch.int32, device=dev)             # (entries behind n[2] are not written)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    work = torch.empty(int(L.spl_seqpack_work_bytes(n_seqs, R, o.strategy)), dtype=torch.uint8, device=dev)
    so = _ffi.SplSeqpackOut(R, rows.data_ptr() if R else work.data_ptr(), _ptr(labels), [_ptr(b) for b in byts], _ptr(mask), _ptr(pos), _ptr(seq),
                            _ptr(place), _ptr(fill), cu.data_ptr(), n.data_ptr(), status.data_ptr())
    rc = L.spl_seqpack_device(tok.handle, ctypes.byref(si), ctypes.byref(o), ctypes.byref(so), work.data_ptr(),
                              torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        _raise_rc(rc, "spl_seqpack_device")
    return PackedRows(rows, labels, mask, pos, seq, byts[0], byts[1], byts[2], byts[3], place, fill, cu, n, status)


def _seqpack_companions(ids: torch.Tensor, labels, byte_arrays):
    names = ("loss_mask", "role_ids", "special_tokens_mask", "extra")
    if labels is not None and (not isinstance(labels, torch.Tensor) or labels.dtype != ids.dtype or labels.shape != ids.shape or
                               not labels.is_contiguous() or labels.device != ids.device):
        raise ValueError("labels must be a contiguous tensor of the dtype, shape and device of the ids")
    for name, b in zip(names, byte_arrays):
        if b is not None and (not isinstance(b, torch.Tensor) or b.dtype != torch.uint8 or b.shape != ids.shape or not b.is_contiguous() or
                              b.device != ids.device):
            raise ValueError(f"{name} must be a contiguous uint8 tensor of the shape and device of the ids")


def seqpack_rows_device(tok: Tokenizer, ids: torch.Tensor, lengths: torch.Tensor, seq_len: int, *, pad_id: int,
                        strategy: str = "best_fit_decreasing", labels: Optional[torch.Tensor] = None, loss_mask: Optional[torch.Tensor] = None,
                        role_ids: Optional[torch.Tensor] = None, special_tokens_mask: Optional[torch.Tensor] = None,
                        extra: Optional[torch.Tensor] = None, padding_side: str = "right", truncation_side: str = "right",
                        ignore_index: int = -100, mask_first: bool = True, fills=SEQPACK_FILLS, max_rows: Optional[int] = None) -> PackedRows:
    """Padded rows -- what pad_device, pair_device and chat_device return: ids [n_seqs, L_in] int32 or int64, lengths int32 [n_seqs],
    padded on `padding_side` -- PACKED: several whole sequences per row of seq_len, none cut in two, two launches on torch's current stream
    (spl_seqpack_device).  A sequence longer than seq_len keeps its head (truncation_side "right") or its tail.  strategy "next_fit"
    keeps the order (a sequence that does not fit the current row opens the next one); "best_fit_decreasing" takes the sequences longest
    first and puts each into the fullest row that still has room (fewer rows; seq_len <= 32768; one GPU lane places the sequences one
    by one, so for tens of thousands of sequences take next_fit).  labels (the ids' dtype) and the uint8 arrays loss_mask, role_ids,
    special_tokens_mask, extra travel with the ids; padding holds pad_id, ignore_index and fills.  mask_first puts ignore_index at every
    sequence's first label (labels are not shifted: the model would learn a sequence's first token from its neighbour's last).  Returns
    PackedRows: input_ids [max_rows, seq_len], labels, attention_mask uint8, position_ids int32 (0 at every sequence start), seq_ids int32
    (-1 in padding), the byte arrays, seq_place int32 [n_seqs, 2] ((row, column); (-1, -1): empty), row_fill int32 [max_rows], cu_seqlens
    int32 (n[2] entries: every sequence start and every padding tail of the flattened rows, then the end -- what a varlen attention call
    takes), n int64 [4] (rows needed, ids placed, entries of cu_seqlens, sequences cut), status int32 [1] (1: a length was out of
    range).  max_rows defaults to n_seqs, which always suffices; with fewer, n[0] still reports the need.  All device tensors, nothing
    synchronises."""
    if not isinstance(ids, torch.Tensor) or ids.dtype not in (torch.int32, torch.int64) or ids.dim() != 2 or not ids.is_contiguous() or not ids.is_cuda:
        raise ValueError("ids must be a contiguous int32 or int64 tensor of rank 2 on a GPU")
    o = _seqpack_opts(seq_len, pad_id, strategy, ignore_index, fills, truncation_side, padding_side, mask_first, ids.dtype, max_rows)
    n_seqs, in_len = int(ids.shape[0]), int(ids.shape[1])
    if not isinstance(lengths, torch.Tensor) or lengths.dtype != torch.int32 or lengths.shape != (n_seqs,) or not lengths.is_contiguous() or \
            lengths.device != ids.device:
        raise ValueError("lengths must be a contiguous int32 tensor of shape [n_seqs] on the device of the ids")
    byts = (loss_mask, role_ids, special_tokens_mask, extra)
    _seqpack_companions(ids, labels, byts)
    if n_seqs and in_len == 0:
        raise ValueError("the input rows have no columns")
    anchor = lengths if n_seqs else torch.zeros(4, dtype=torch.int32, device=ids.device)         # (an empty tensor has no address)
    si = _ffi.SplSeqpackIn(n_seqs, in_len, _ptr(ids), anchor.data_ptr(), None, _ptr(labels), [_ptr(b) for b in byts])
    return _seqpack_call(tok, o, si, ids.device, n_seqs, labels is not None, [b is not None for b in byts], ids.dtype, max_rows)


def seqpack_csr_device(tok: Tokenizer, ids: torch.Tensor, offsets: torch.Tensor, n_seqs: int, seq_len: int, *, pad_id: int,
                       strategy: str = "best_fit_decreasing", labels: Optional[torch.Tensor] = None, loss_mask: Optional[torch.Tensor] = None,
                       role_ids: Optional[torch.Tensor] = None, special_tokens_mask: Optional[torch.Tensor] = None,
                       extra: Optional[torch.Tensor] = None, truncation_side: str = "right", ignore_index: int = -100, mask_first: bool = True,
                       fills=SEQPACK_FILLS, dtype: torch.dtype = torch.int32, max_rows: Optional[int] = None) -> PackedRows:
    """seqpack_rows_device for a CSR -- what encode_device leaves: ids int32 [capacity], offsets int64 [at least n_seqs + 1], ABSOLUTE into
    ids; labels (int32) and the uint8 arrays in the layout of the ids.  dtype: that of the rows returned.  Same return."""
    o = _seqpack_opts(seq_len, pad_id, strategy, ignore_index, fills, truncation_side, "right", mask_first, dtype, max_rows)
    n_seqs = int(n_seqs)
    if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int32 or ids.dim() != 1 or not ids.is_contiguous() or not ids.is_cuda:
        raise ValueError("ids must be a contiguous int32 tensor of rank 1 on a GPU")
    if not isinstance(offsets, torch.Tensor) or offsets.dtype != torch.int64 or offsets.dim() != 1 or not offsets.is_contiguous() or n_seqs < 0 or \
            offsets.shape[0] < n_seqs + 1 or offsets.device != ids.device:
        raise ValueError("offsets must be a contiguous int64 tensor of at least n_seqs + 1 entries on the device of the ids")
    byts = (loss_mask, role_ids, special_tokens_mask, extra)
    _seqpack_companions(ids, labels, byts)
    si = _ffi.SplSeqpackIn(n_seqs, 0, ids.data_ptr(), None, offsets.data_ptr(), _ptr(labels), [_ptr(b) for b in byts])
    return _seqpack_call(tok, o, si, ids.device, n_seqs, labels is not None, [b is not None for b in byts], dtype, max_rows)


def seqpack_trim(p: PackedRows) -> PackedRows:
    """p cut to the rows that are used and the cu_seqlens entries that are written: ONE synchronisation (n goes to the host)."""
    n = p.n.tolist()
    r = min(int(n[0]), int(p.input_ids.shape[0]))
    cut = lambda t: None if t is None else t[:r]
    return PackedRows(cut(p.input_ids), cut(p.labels), cut(p.attention_mask), cut(p.position_ids), cut(p.seq_ids), cut(p.loss_mask),
                      cut(p.role_ids), cut(p.special_tokens_mask), cut(p.extra), p.seq_place, cut(p.row_fill), p.cu_seqlens[:int(n[2])], p.n,
                      p.status)


# ---------------------------------------------------------------------------------------------- device-resident decode
def _max_bytes(max_bytes) -> int:
    if isinstance(max_bytes, bool) or not isinstance(max_bytes, (int, np.integer)) or not 0 <= int(max_bytes) < (1 << 62):
        raise ValueError(f"max_bytes must be an integer in 0 .. 2**62 - 1, not {max_bytes!r}")
    return (int(max_bytes) + 15) // 16 * 16


def check_decode_args(ids, offsets=None, lengths=None, *, rows: bool, max_bytes=0, padding_side: str = "right") -> None:
    """ValueError for a dtype, rank, device, layout, side string or size that decode_device / decode_rows_device would refuse -- before
    anything goes to the device."""
    _side("padding_side", padding_side)
    _max_bytes(max_bytes)
    if not isinstance(ids, torch.Tensor) or ids.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"the ids must be a torch tensor of dtype int32 or int64, not {getattr(ids, 'dtype', type(ids))}")
    if not ids.is_contiguous():
        raise ValueError("the ids must be contiguous")
    other = None
    if rows:
        if ids.dim() != 2:
            raise ValueError(f"the rows must have rank 2 ([batch, steps]), not {ids.dim()}")
        if ids.shape[1] >= (1 << 32) or ids.shape[0] >= (1 << 31):
            raise ValueError("the rows must be fewer than 2**31 and shorter than 2**32")
        if lengths is not None:
            if not isinstance(lengths, torch.Tensor) or lengths.dtype != torch.int32 or lengths.dim() != 1 or \
                    lengths.shape[0] != ids.shape[0] or not lengths.is_contiguous():
                raise ValueError("lengths must be a contiguous int32 tensor of shape [batch]")
            other = ("lengths", lengths)
    else:
        if ids.dim() != 1:
            raise ValueError(f"the ids of a CSR must have rank 1, not {ids.dim()}")
        if not isinstance(offsets, torch.Tensor) or offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.shape[0] < 1 or \
                not offsets.is_contiguous():
            raise ValueError("offsets must be a contiguous int64 tensor of shape [n_docs + 1]")
        if offsets.shape[0] - 1 >= (1 << 31):
            raise ValueError("the documents must be fewer than 2**31")
        other = ("offsets", offsets)
    if not ids.is_cuda:
        raise ValueError("the ids must be on a GPU (device-resident decode takes no host tensor)")
    if other is not None and other[1].device != ids.device:
        raise ValueError(f"{other[0]} must be on the device of the ids")


def decode_reserve(tok: Tokenizer, max_ids: int) -> None:
    """spl_decode_reserve_device: the decode tables on the device and scratch for max_ids ids (rows: batch * steps); decode_device /
    decode_rows_device calls within that size then neither allocate nor synchronise."""
    rc = _ffi.lib().spl_decode_reserve_device(tok.handle, int(max_ids))
    if rc != 0:
        _raise_rc(rc, "spl_decode_reserve_device")


def _decode_call(tok: Tokenizer, ids: torch.Tensor, n_ids_cap: int, offsets, lengths, n_docs: int, o, max_bytes: int):
    dev = ids.device
    out = torch.empty(_max_bytes(max_bytes), dtype=torch.uint8, device=dev)
    out_off = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)           # (every offset is written by the kernel)
    rc = _ffi.lib().spl_decode_batch_device(tok.handle, ids.data_ptr() if ids.numel() else None, n_ids_cap,
                                            offsets.data_ptr() if offsets is not None else None,
                                            lengths.data_ptr() if lengths is not None else None, n_docs, ctypes.byref(o),
                                            out.data_ptr() if out.numel() else None, out.numel(), out_off.data_ptr(),
                                            torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        _raise_rc(rc, "spl_decode_batch_device")
    return out, out_off


def decode_device(tok: Tokenizer, ids: torch.Tensor, offsets: torch.Tensor, *, max_bytes: int,
                  skip_special_tokens: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """A CSR of ids in HBM (ids int32 / int64 [capacity], offsets int64 [n_docs + 1], offsets[0] == 0 -- what encode_device leaves) to a
    bytes CSR in HBM, on torch's current stream (spl_decode_batch_device); nothing synchronises.  ids.numel() is only an upper bound of
    the id count.  Returns (bytes uint8 [max_bytes rounded up to 16], out_off int64 [n_docs + 1]); out_off[-1] is the byte count NEEDED:
    bytes beyond the buffer are dropped, compare the two."""
    check_decode_args(ids, offsets, rows=False, max_bytes=max_bytes)
    flags = (_ffi.SPL_DECODE_I64 if ids.dtype == torch.int64 else 0) | (_ffi.SPL_DECODE_SKIP_SPECIAL if skip_special_tokens else 0)
    return _decode_call(tok, ids, ids.numel(), offsets, None, offsets.shape[0] - 1, _ffi.SplDecodeOpts(flags, 0), max_bytes)


def decode_rows_device(tok: Tokenizer, rows: torch.Tensor, lengths: Optional[torch.Tensor] = None, *, max_bytes: int,
                       padding_side: str = "right", skip_special_tokens: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """Rows [batch, steps] int32 / int64 in HBM (what a sampler leaves, or pad_device) to a bytes CSR in HBM, one document per row.  With
    lengths (int32 [batch], as pad_device returns them) a row's valid entries are its first lengths[r] -- padding_side "left": its last --
    and the others contribute nothing; an int64 value outside 0 .. 2**32 - 1 (-1, -100) is no id and contributes nothing.  Same return
    as decode_device; nothing synchronises."""
    check_decode_args(rows, None, lengths, rows=True, max_bytes=max_bytes, padding_side=padding_side)
    flags = (_ffi.SPL_DECODE_I64 if rows.dtype == torch.int64 else 0) | (_ffi.SPL_DECODE_SKIP_SPECIAL if skip_special_tokens else 0) | \
        (_ffi.SPL_DECODE_PAD_LEFT if padding_side == "left" else 0)
    n_docs, row_len = int(rows.shape[0]), int(rows.shape[1])
    if row_len == 0:                                  # (no entry anywhere: every document is empty; row_len 0 would mean CSR mode)
        out = torch.empty(_max_bytes(max_bytes), dtype=torch.uint8, device=rows.device)
        return out, torch.zeros(n_docs + 1, dtype=torch.int64, device=rows.device)
    return _decode_call(tok, rows, 0, None, lengths, n_docs, _ffi.SplDecodeOpts(flags, row_len), max_bytes)


# ---------------------------------------------------------------------------------------------- token spans (byte and character offsets per id)
def _span_dtype(dtype) -> int:
    if dtype not in (torch.int32, torch.int64):
        raise ValueError(f"dtype must be torch.int32 or torch.int64, not {dtype}")
    return _ffi.SPL_SPANS_I64 if dtype == torch.int64 else 0


def _spans_call(tok: Tokenizer, ids: torch.Tensor, n_ids_cap: int, offsets, lengths, n_docs: int, o, slots: int, chars: bool, dtype):
    dev = ids.device
    new = lambda *shape, dt: torch.empty(*shape, dtype=dt, device=dev)          # (every entry is written by the kernels)
    byte_span = new(slots, 2, dt=dtype)
    char_span = new(slots, 2, dt=dtype) if chars else None
    byte_off = new(n_docs + 1, dt=torch.int64)
    char_off = new(n_docs + 1, dt=torch.int64) if chars else None
    rc = _ffi.lib().spl_token_spans_device(tok.handle, _ptr(ids), n_ids_cap, _ptr(offsets), _ptr(lengths), n_docs, ctypes.byref(o),
                                           _span_dtype(dtype), _ptr(byte_span), _ptr(char_span), byte_off.data_ptr(), _ptr(char_off),
                                           torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        _raise_rc(rc, "spl_token_spans_device")
    return byte_span, char_span, byte_off, char_off


def spans_device(tok: Tokenizer, ids: torch.Tensor, offsets: torch.Tensor, *, chars: bool = True, dtype=torch.int32,
                 skip_special_tokens: bool = False):
    """Where every id of a CSR in HBM (decode_device's input: what encode_device leaves) lies in the text decode_device writes for it, on
    torch's current stream (spl_token_spans_device); nothing synchronises.  Returns (byte_span [ids.numel(), 2], char_span or None,
    byte_off int64 [n_docs + 1], char_off or None): a span counts from its document's start -- bytes, and characters by tiktoken's
    decode_with_offsets rule (str indices for valid UTF-8) -- and byte_off is decode_device's out_off, entry for entry.  Slots at or
    beyond offsets[-1] hold (0, 0).  The spans describe the DECODED text: where an encode dropped bytes, byte_off[d + 1] - byte_off[d]
    differs from the text's length."""
    _span_dtype(dtype)
    check_decode_args(ids, offsets, rows=False)
    flags = (_ffi.SPL_DECODE_I64 if ids.dtype == torch.int64 else 0) | (_ffi.SPL_DECODE_SKIP_SPECIAL if skip_special_tokens else 0)
    return _spans_call(tok, ids, ids.numel(), offsets, None, offsets.shape[0] - 1, _ffi.SplDecodeOpts(flags, 0), ids.numel(), chars, dtype)


def spans_rows_device(tok: Tokenizer, rows: torch.Tensor, lengths: Optional[torch.Tensor] = None, *, padding_side: str = "right",
                      chars: bool = True, dtype=torch.int32, skip_special_tokens: bool = False):
    """spans_device for rows [batch, steps] (decode_rows_device's input), one document per row: spans [batch * steps, 2] in row-major
    order; a padding entry is a zero-length slot of its row (the empty span at its position)."""
    _span_dtype(dtype)
    check_decode_args(rows, None, lengths, rows=True, padding_side=padding_side)
    flags = (_ffi.SPL_DECODE_I64 if rows.dtype == torch.int64 else 0) | (_ffi.SPL_DECODE_SKIP_SPECIAL if skip_special_tokens else 0) | \
        (_ffi.SPL_DECODE_PAD_LEFT if padding_side == "left" else 0)
    n_docs, row_len = int(rows.shape[0]), int(rows.shape[1])
    if row_len == 0:                                  # (no entry anywhere: every document is empty; row_len 0 would mean CSR mode)
        z = lambda: torch.zeros(n_docs + 1, dtype=torch.int64, device=rows.device)
        e = lambda: torch.empty(0, 2, dtype=dtype, device=rows.device)
        return e(), (e() if chars else None), z(), (z() if chars else None)
    return _spans_call(tok, rows, 0, None, lengths, n_docs, _ffi.SplDecodeOpts(flags, row_len), n_docs * row_len, chars, dtype)


# ---------------------------------------------------------------------------------------------- batched streaming decode (per-sequence UTF-8 state)
def _stream_mode(errors: str) -> int:
    if errors not in ("hold", "replace"):
        raise ValueError(f"errors must be 'hold' or 'replace', not {errors!r}")
    return _ffi.SPL_STREAM_REPLACE if errors == "replace" else 0


def check_stream_args(ids, lengths, state, *, errors: str = "hold", final=None, max_bytes=0, state_out=None) -> None:
    """ValueError for a mode string, dtype, rank, shape, layout, size or device that stream_decode_device would refuse -- before anything goes
    to the device."""
    _stream_mode(errors)
    _max_bytes(max_bytes)
    if not isinstance(ids, torch.Tensor) or ids.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"the ids must be a torch tensor of dtype int32 or int64, not {getattr(ids, 'dtype', type(ids))}")
    if ids.dim() not in (1, 2):
        raise ValueError(f"the ids must have rank 1 ([batch]: one id per sequence) or 2 ([batch, steps]), not {ids.dim()}")
    if not ids.is_contiguous():
        raise ValueError("the ids must be contiguous")
    B = int(ids.shape[0])
    if ids.dim() == 2 and not 1 <= ids.shape[1] < (1 << 32):
        raise ValueError("a row must hold at least one id and fewer than 2**32")
    if B >= (1 << 31):
        raise ValueError("the sequences must be fewer than 2**31")
    others = []

    if lengths is not None:
        others.append(_vec("lengths", lengths, B, (torch.int32,), "int32"))
    others.append(_vec("state", state, B, (torch.int64,), "int64"))
    if state_out is not None:
        others.append(_vec("state_out", state_out, B, (torch.int64,), "int64"))
    if final is not None and not isinstance(final, bool):
        others.append(_vec("final", final, B, (torch.uint8, torch.bool), "uint8 or bool"))
    if not ids.is_cuda:
        raise ValueError("the ids must be on a GPU (the device-side streaming decode takes no host tensor)")
    for name, t in others:
        if t.device != ids.device:
            raise ValueError(f"{name} must be on the device of the ids")


def stream_reserve(tok: Tokenizer, max_seqs: int) -> None:
    """spl_stream_reserve_device: the decode tables on the device and scratch for max_seqs sequences; stream_decode_device calls within that
    size then neither allocate nor synchronise."""
    rc = _ffi.lib().spl_stream_reserve_device(tok.handle, int(max_seqs))
    if rc != 0:
        _raise_rc(rc, "spl_stream_reserve_device")


def stream_decode_device(tok: Tokenizer, ids: torch.Tensor, lengths: Optional[torch.Tensor], state: torch.Tensor, *, errors: str = "hold",
                         final=None, max_bytes: int, skip_special_tokens: bool = False,
                         state_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """One step of B streaming decoders on the GPU (spl_stream_decode_device), on torch's current stream; nothing synchronises.  ids [B] or
    [B, K] int32 / int64 (what a sampler leaves: a sequence's first lengths[b] entries count, all of them with lengths None; an int64
    value outside 0 .. 2**32 - 1 is no id); state int64 [B], one word per sequence as include/splintr_hip.h lays it out (0: a fresh
    decoder).  errors "hold" is the host StreamingDecoder step for step (invalid bytes stall a sequence for ever), "replace" emits U+FFFD
    for them.  final: None, True (every sequence) or a uint8 / bool tensor [B]: pending bytes leave as one U+FFFD behind this step's ids.
    Returns (bytes uint8 [max_bytes rounded up to 16], out_off int64 [B + 1], state_out int64 [B]); out_off[-1] is the byte count NEEDED,
    bytes beyond the buffer are dropped -- and the state has advanced all the same: pass a state_out other than state where the call may
    have to be repeated with a larger buffer (state_out None: a new tensor; state_out may be state itself)."""
    check_stream_args(ids, lengths, state, errors=errors, final=final, max_bytes=max_bytes, state_out=state_out)
    dev = ids.device
    B = int(ids.shape[0])
    K = int(ids.shape[1]) if ids.dim() == 2 else 1
    flags = (_ffi.SPL_DECODE_I64 if ids.dtype == torch.int64 else 0) | (_ffi.SPL_DECODE_SKIP_SPECIAL if skip_special_tokens else 0)
    sflags = _stream_mode(errors) | (_ffi.SPL_STREAM_FINAL_ALL if final is True else 0)
    out = torch.empty(_max_bytes(max_bytes), dtype=torch.uint8, device=dev)
    out_off = torch.empty(B + 1, dtype=torch.int64, device=dev)                # (every offset and every state word is written by the kernels)
    if state_out is None:
        state_out = torch.empty(B, dtype=torch.int64, device=dev)
    o = _ffi.SplDecodeOpts(flags, K)
    # (a null state pointer is refused by the library: an empty batch passes the offsets' address, which nothing dereferences)
    rc = _ffi.lib().spl_stream_decode_device(tok.handle, _ptr(ids), _ptr(lengths), B, ctypes.byref(o), sflags, _ptr(final),
                                             _ptr(state) or out_off.data_ptr(), _ptr(state_out) or out_off.data_ptr(), _ptr(out), out.numel(),
                                             out_off.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        _raise_rc(rc, "spl_stream_decode_device")
    return out, out_off, state_out


# ---------------------------------------------------------------------------------------------- stop strings (per-sequence match state)
def _stop_table_host(stops) -> np.ndarray:
    if isinstance(stops, (str, bytes, bytearray)) or not hasattr(stops, "__iter__"):
        raise ValueError("stops must be a list of str or bytes")
    stops = list(stops)
    if len(stops) > _ffi.SPL_STOP_SLOTS:
        raise ValueError(f"at most {_ffi.SPL_STOP_SLOTS} stops fit the table, not {len(stops)}")
    tab = np.zeros(_ffi.SPL_STOP_TABLE_BYTES, dtype=np.uint8)
    for s, x in enumerate(stops):
        if isinstance(x, str):
            x = x.encode("utf-8")
        elif not isinstance(x, (bytes, bytearray)):
            raise ValueError(f"stop {s} must be str or bytes, not {type(x).__name__}")
        if not 1 <= len(x) <= _ffi.SPL_STOP_MAX_LEN:
            raise ValueError(f"stop {s} must have 1 .. {_ffi.SPL_STOP_MAX_LEN} bytes, not {len(x)}")
        tab[_ffi.SPL_STOP_MAX_LEN * s:_ffi.SPL_STOP_MAX_LEN * s + len(x)] = np.frombuffer(bytes(x), dtype=np.uint8)
        tab[_ffi.SPL_STOP_SLOTS * _ffi.SPL_STOP_MAX_LEN + s] = len(x)
    return tab


def stop_table(stops, device=None) -> torch.Tensor:
    """The stop table of spl_stop_match_device on the device (default: the current GPU): uint8 [4160], slot s = stops[s] (str: its UTF-8).
    ValueError for an empty stop, one over 64 bytes, or more than 64 stops.  The tensor is the caller's: a slot may be rewritten (a
    stream-ordered copy) only while no live sequence's mask names it."""
    tab = _stop_table_host(stops)
    return torch.from_numpy(tab).to(torch.device("cuda") if device is None else device)


def check_stop_args(in_bytes, in_off, state, table, *, mask=None, final=None, max_bytes=0, state_out=None) -> None:
    """ValueError for a dtype, rank, shape, layout, size or device that stop_match_device would refuse -- before anything goes to the
    device."""
    _max_bytes(max_bytes)
    if not isinstance(in_bytes, torch.Tensor) or in_bytes.dtype != torch.uint8 or in_bytes.dim() != 1 or not in_bytes.is_contiguous():
        raise ValueError("in_bytes must be a contiguous uint8 tensor of rank 1")
    if not isinstance(in_off, torch.Tensor) or in_off.dtype != torch.int64 or in_off.dim() != 1 or in_off.shape[0] < 1 or not in_off.is_contiguous():
        raise ValueError("in_off must be a contiguous int64 tensor of shape [batch + 1]")
    B = int(in_off.shape[0]) - 1
    if B >= (1 << 31):
        raise ValueError("the sequences must be fewer than 2**31")
    if not isinstance(table, torch.Tensor) or table.dtype != torch.uint8 or table.shape != (_ffi.SPL_STOP_TABLE_BYTES,) or not table.is_contiguous():
        raise ValueError(f"table must be a contiguous uint8 tensor of shape [{_ffi.SPL_STOP_TABLE_BYTES}] (stop_table)")
    others = [("in_off", in_off), ("table", table)]

    def rows(name, t):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.shape != (B, _ffi.SPL_STOP_STATE_WORDS) or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous int64 tensor of shape [batch, {_ffi.SPL_STOP_STATE_WORDS}]")
        others.append((name, t))

    rows("state", state)
    if state_out is not None:
        rows("state_out", state_out)
    if mask is not None:
        others.append(_vec("mask", mask, B, (torch.int64,), "int64"))
    if final is not None and not isinstance(final, bool):
        others.append(_vec("final", final, B, (torch.uint8, torch.bool), "uint8 or bool"))
    if not in_bytes.is_cuda:
        raise ValueError("in_bytes must be on a GPU (the device-side stop match takes no host tensor)")
    for name, t in others:
        if t.device != in_bytes.device:
            raise ValueError(f"{name} must be on the device of in_bytes")


def stop_reserve(tok: Tokenizer, max_seqs: int) -> None:
    """spl_stop_reserve_device: scratch for max_seqs sequences; stop_match_device calls within that size then neither allocate nor
    synchronise."""
    rc = _ffi.lib().spl_stop_reserve_device(tok.handle, int(max_seqs))
    if rc != 0:
        _raise_rc(rc, "spl_stop_reserve_device")


def stop_match_device(tok: Tokenizer, in_bytes: torch.Tensor, in_off: torch.Tensor, state: torch.Tensor, table: torch.Tensor, *, mask=None,
                      final=None, include_stop: bool = False, max_bytes: int,
                      state_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Stop strings for B streaming sequences on the GPU (spl_stop_match_device), on torch's current stream; nothing synchronises.
    in_bytes uint8 / in_off int64 [B + 1]: a bytes CSR -- stream_decode_device's as it is (offsets beyond in_bytes are clamped); state int64
    [B, 10], one row per sequence as include/splintr_hip.h lays it out (zeros: fresh); table: stop_table(...); mask int64 [B], bit s: slot
    s applies to the sequence (None: every slot to everyone).  final: None, True (every sequence) or a uint8 / bool tensor [B]: the held
    bytes leave too.  Returns (bytes uint8 [max_bytes rounded up to 16], out_off int64 [B + 1], hit int32 [B]: -1 or the slot, state_out
    int64 [B, 10]); out_off[-1] is the byte count NEEDED, bytes beyond the buffer are dropped -- and the state has advanced all the same:
    pass a state_out other than state where the call may have to be repeated (None: a new tensor; state_out may be state itself)."""
    check_stop_args(in_bytes, in_off, state, table, mask=mask, final=final, max_bytes=max_bytes, state_out=state_out)
    dev = in_bytes.device
    B = int(in_off.shape[0]) - 1
    flags = (_ffi.SPL_STOP_INCLUDE if include_stop else 0) | (_ffi.SPL_STOP_FINAL_ALL if final is True else 0)
    out = torch.empty(_max_bytes(max_bytes), dtype=torch.uint8, device=dev)
    out_off = torch.empty(B + 1, dtype=torch.int64, device=dev)                # (every offset, hit and state word is written by the kernels)
    hit = torch.empty(max(B, 1), dtype=torch.int32, device=dev)[:B]
    if state_out is None:
        state_out = torch.empty((B, _ffi.SPL_STOP_STATE_WORDS), dtype=torch.int64, device=dev)
    # (null state and hit pointers are refused by the library: an empty batch passes the offsets' address, which nothing dereferences)
    rc = _ffi.lib().spl_stop_match_device(tok.handle, _ptr(in_bytes), in_bytes.numel(), in_off.data_ptr(), B, table.data_ptr(), _ptr(mask),
                                          _ptr(final), flags, _ptr(state) or out_off.data_ptr(), _ptr(state_out) or out_off.data_ptr(),
                                          _ptr(out), out.numel(), out_off.data_ptr(), _ptr(hit) or out_off.data_ptr(),
                                          torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        _raise_rc(rc, "spl_stop_match_device")
    return out, out_off, hit, state_out


class DeviceStreamingDecoder:
    """`tokenizer.device_streaming_decoder(batch_size)`: B streaming decoders whose state lives on the GPU, one word per sequence.  The
    host classes of splintr_amd.streaming decode one id per Python call; this one takes a whole step of the batch as a device tensor.
    errors "hold" emits exactly what B host decoders emit (ByteLevel vocabularies: byte_level_streaming_decoder, others:
    streaming_decoder); "replace" never stalls.  stop: stop strings (stop_table's rules) -- every step's text then goes through
    stop_match_device on the same stream: the text is cut at the first stop (include_stop_str_in_output: behind it), text that may still
    become one is held back, a sequence that hit emits nothing more, and `finished` / `stop_hit` are device tensors."""

    BYTES_PER_ID = 8           # first guess of a step's buffer; a short buffer repeats the step once with the exact need

    def __init__(self, tok: Tokenizer, batch_size: int, *, errors: str = "hold", skip_special_tokens: bool = False, stop=None,
                 include_stop_str_in_output: bool = False):
        _stream_mode(errors)
        if isinstance(batch_size, bool) or not isinstance(batch_size, (int, np.integer)) or not 0 <= int(batch_size) < (1 << 31):
            raise ValueError(f"batch_size must be an integer in 0 .. 2**31 - 1, not {batch_size!r}")
        stop_tab = None if stop is None else _stop_table_host(stop)
        self._tok, self._errors, self._skip = tok, errors, bool(skip_special_tokens)
        self.batch_size = int(batch_size)
        dev = torch.device("cuda", tok._device)
        self._state = torch.zeros(self.batch_size, dtype=torch.int64, device=dev)      # the current words ...
        self._spare = torch.zeros(self.batch_size, dtype=torch.int64, device=dev)      # ... and where the next step leaves its own
        stream_reserve(tok, self.batch_size)
        self._stop_table = None
        if stop_tab is not None:
            rows = (self.batch_size, _ffi.SPL_STOP_STATE_WORDS)
            self._stop_table = torch.from_numpy(stop_tab).to(dev)
            self._include = bool(include_stop_str_in_output)
            self._sstate = torch.zeros(rows, dtype=torch.int64, device=dev)             # the stop rows, kept the same way
            self._sspare = torch.zeros(rows, dtype=torch.int64, device=dev)
            self._smask = None                                                          # (every slot applies to every sequence)
            self._prev_decoded = (torch.empty(0, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))
            stop_reserve(tok, self.batch_size)

    def step_device(self, ids: torch.Tensor, lengths: Optional[torch.Tensor] = None, *, final=None, max_bytes: Optional[int] = None):
        """Tensors only, nothing synchronises: one step -> (bytes, out_off int64 [B + 1]) on the device; out_off[-1] is the need.  The
        state advances whatever max_bytes is (default 8 bytes per id, 16 at least).  With stops the two calls run back to back on the
        current stream and what comes back is the RELEASED text (its buffer holds max_bytes and the 63 bytes a sequence can have held).
        The match reads what the decode WROTE: if the decode needed more than max_bytes, the text beyond it never reached the match, the
        stop rows have advanced on the cut text, and the returned out_off[-1] does not show it.  `decode_overflowed` (a device bool, no
        synchronisation) is that signal, `decode_need` the bytes the decode needed; a caller of this path either sizes max_bytes for the
        worst case -- ids per sequence x Tokenizer's longest token, x B -- or reads the flag with whatever it reads next and repeats
        the step from a state it kept (add_tokens does exactly that)."""
        if isinstance(ids, torch.Tensor) and ids.shape[:1] != (self.batch_size,):
            raise ValueError(f"the ids must have {self.batch_size} rows")
        if max_bytes is None:
            max_bytes = max(16, self.BYTES_PER_ID * ids.numel()) if isinstance(ids, torch.Tensor) else 16
        out, off, _ = stream_decode_device(self._tok, ids, lengths, self._state, errors=self._errors, final=final, max_bytes=max_bytes,
                                           skip_special_tokens=self._skip, state_out=self._spare)
        self._prev_args = (ids, lengths, final)
        self._state, self._spare = self._spare, self._state
        if self._stop_table is None:
            return out, off
        self._prev_decoded = (out, off)
        out, off = self._stop_step(out, off, final, out.numel() + (_ffi.SPL_STOP_MAX_LEN - 1) * self.batch_size, self._sstate, self._sspare)
        self._sstate, self._sspare = self._sspare, self._sstate
        return out, off

    def _stop_step(self, out, off, final, max_bytes, state, state_out):
        out, off, _, _ = stop_match_device(self._tok, out, off, state, self._stop_table, mask=self._smask, final=final,
                                           include_stop=self._include, max_bytes=max_bytes, state_out=state_out)
        return out, off

    def _texts(self, out, off):
        if self._stop_table is not None:
            d_out, d_off = self._prev_decoded
            d_need, need = torch.stack((d_off[-1], off[-1])).tolist()
            if d_need > d_out.numel() or need > out.numel():       # both calls once more from the kept states: the decode with its exact need,
                ids, lengths, final = self._prev_args              # the match with what that and the held bytes can come to at most
                d_out, d_off, _ = stream_decode_device(self._tok, ids, lengths, self._spare, errors=self._errors, final=final,
                                                       max_bytes=d_need, skip_special_tokens=self._skip, state_out=self._state)
                out, off = self._stop_step(d_out, d_off, final, d_need + (_ffi.SPL_STOP_MAX_LEN - 1) * self.batch_size, self._sspare,
                                           self._sstate)
                need = int(off[-1].item())                         # (a match that read a cut input has counted less)
        else:
            need = int(off[-1].item())
            if need > out.numel():                                     # the step once more from the kept state_in, with the exact need
                ids, lengths, final = self._prev_args
                out, off, _ = stream_decode_device(self._tok, ids, lengths, self._spare, errors=self._errors, final=final, max_bytes=need,
                                                   skip_special_tokens=self._skip, state_out=self._state)
        raw = out[:need].cpu().numpy().tobytes()
        o = off.cpu().tolist()
        return [raw[o[i]:o[i + 1]].decode("utf-8") if o[i + 1] > o[i] else None for i in range(len(o) - 1)]

    def add_tokens(self, ids: torch.Tensor, lengths: Optional[torch.Tensor] = None, *, max_bytes: Optional[int] = None):
        """ids [B] or [B, K] on the GPU -> list of B entries: the text that leaves for sequence b now (with stops: the released text), None
        where nothing does (as the host class).  One copy of the bytes and one of the offsets to the host."""
        return self._texts(*self.step_device(ids, lengths, max_bytes=max_bytes))

    def flush(self, rows=None):
        """What is pending leaves as U+FFFD -- for every sequence, or for those of `rows` (a uint8 / bool tensor [B], or indices) -- and
        their state becomes fresh; a stalled sequence (errors "hold") gives None and stays stalled (see `stalled`; reset it).  With stops
        the text held back leaves too (a sequence that hit stays finished and gives None)."""
        dev = self._state.device
        none = torch.zeros(self.batch_size, dtype=torch.int32, device=dev)
        ids = torch.zeros((self.batch_size, 1), dtype=torch.int32, device=dev)
        return self._texts(*self.step_device(ids, none, final=True if rows is None else self._mask(rows)))

    def _mask(self, rows):
        dev = self._state.device
        if isinstance(rows, torch.Tensor) and rows.dtype in (torch.uint8, torch.bool) and rows.shape == (self.batch_size,):
            return rows.to(dev).contiguous()
        m = torch.zeros(self.batch_size, dtype=torch.uint8, device=dev)
        m[torch.as_tensor(rows, dtype=torch.long, device=dev)] = 1
        return m

    def reset(self, rows=None) -> None:
        if rows is None:
            self._state.zero_()
            if self._stop_table is not None:
                self._sstate.zero_()
        else:
            m = self._mask(rows).bool()
            self._state[m] = 0
            if self._stop_table is not None:
                self._sstate[m] = 0

    def _need_stops(self):
        if self._stop_table is None:
            raise ValueError("this decoder was made without stop strings (stop=None)")

    def set_stop_mask(self, rows, mask) -> None:
        """Which stops apply to the sequences of `rows` (a uint8 / bool tensor [B], or indices; None: all): mask is an int whose bit s
        says that stop s applies, or an int64 tensor of one such word per selected sequence.  For sequences that are fresh (reset):
        what a live sequence holds back was held for the stops its mask named."""
        self._need_stops()
        if self._smask is None:
            self._smask = torch.full((self.batch_size,), -1, dtype=torch.int64, device=self._state.device)
        if isinstance(mask, (int, np.integer)) and not isinstance(mask, bool):
            mask = int(mask) & 0xFFFFFFFFFFFFFFFF
            mask = mask - (1 << 64) if mask >= (1 << 63) else mask
        elif not isinstance(mask, torch.Tensor) or mask.dtype != torch.int64:
            raise ValueError("mask must be an int or an int64 tensor")
        if rows is None:
            self._smask[:] = mask
        else:
            self._smask[self._mask(rows).bool()] = mask

    def allowed_mask(self, out: Optional[torch.Tensor] = None, *, and_into: bool = False, n_words: Optional[int] = None):
        """The ids the next step may draw without stalling a sequence (errors "hold") or putting U+FFFD into its text ("replace"):
        utf8_mask_device over the decoder's own state words and skip_special_tokens -> (mask int32 [B, n_words], live uint8 [B]).  out:
        the mask to write (and_into: to AND the rows into -- a TokenHealer's mask, a grammar's).  Nothing synchronises."""
        return utf8_mask_device(self._tok, self._state, n_words=n_words, skip_special_tokens=self._skip, out=out, and_into=and_into)

    @property
    def state(self) -> torch.Tensor:
        return self._state

    @property
    def stop_state(self) -> torch.Tensor:
        """int64 [B, 10] on the device: the stop rows (include/splintr_hip.h)"""
        self._need_stops()
        return self._sstate

    @property
    def decode_need(self) -> torch.Tensor:
        """int64 scalar on the device (no synchronisation): the bytes the last step's DECODE needed -- what out_off[-1] is without stops"""
        self._need_stops()
        return self._prev_decoded[1][-1]

    @property
    def decode_overflowed(self) -> torch.Tensor:
        """bool scalar on the device (no synchronisation): the last step's decode needed more than its buffer, so the match saw cut text"""
        self._need_stops()
        return self._prev_decoded[1][-1] > self._prev_decoded[0].numel()

    @property
    def finished(self) -> torch.Tensor:
        """bool [B] on the device, read from the stop rows (no synchronisation): the sequence has hit a stop"""
        self._need_stops()
        return ((self._sstate[:, 0] >> 16) & 1).bool()

    @property
    def stop_hit(self) -> torch.Tensor:
        """int32 [B] on the device, read from the stop rows (no synchronisation): the stop that was hit, -1 where none was"""
        self._need_stops()
        w = self._sstate[:, 0]
        return torch.where((w >> 16) & 1 != 0, (w >> 24) & 63, torch.full_like(w, -1)).to(torch.int32)

    @property
    def pending_bytes(self) -> torch.Tensor:
        """int64 [B] on the device: the host class's pending_bytes per sequence"""
        s = self._state
        return torch.where((s >> 26) & 1 != 0, (s >> 32) & 0xFFFFFFFF, (s >> 24) & 3)

    @property
    def stalled(self) -> torch.Tensor:
        return ((self._state >> 26) & 1).bool()

    def __repr__(self) -> str:
        return f"DeviceStreamingDecoder(batch_size={self.batch_size}, errors={self._errors!r})"


# ---------------------------------------------------------------------------------------------- token healing (allowed-token bitmasks from byte prefixes)
def heal_reserve(tok: Tokenizer, max_seqs: int) -> None:
    """spl_heal_reserve_device: the decode tables, the sorted order of the ordinary ids and their prefix order on the device, and scratch
    for max_seqs sequences; heal_begin_device / heal_step_device calls within that size then neither allocate nor synchronise."""
    rc = _ffi.lib().spl_heal_reserve_device(tok.handle, int(max_seqs))
    if rc != 0:
        _raise_rc(rc, "spl_heal_reserve_device")


def heal_n_words(tok: Tokenizer) -> int:
    """The words of a mask row that cover every id the tokenizer knows (specials included)."""
    return (tok.vocab_size + 31) // 32


def heal_state_from_prefixes(prefixes, device=None) -> torch.Tensor:
    """State rows int64 [len(prefixes), 9] for fresh sequences whose pending prefix is the given text (str: its UTF-8; empty: free), built
    on the host -- "the answer must begin with this text": heal_step_device with ids None then writes the first masks.  ValueError for a
    prefix over 64 bytes.  The tensor goes to `device` (default: the current GPU)."""
    if isinstance(prefixes, (str, bytes, bytearray)) or not hasattr(prefixes, "__iter__"):
        raise ValueError("prefixes must be a list of str or bytes")
    prefixes = list(prefixes)
    rows = np.zeros((len(prefixes), _ffi.SPL_HEAL_STATE_WORDS), dtype=np.uint64)
    for b, x in enumerate(prefixes):
        if isinstance(x, str):
            x = x.encode("utf-8")
        elif not isinstance(x, (bytes, bytearray)):
            raise ValueError(f"prefix {b} must be str or bytes, not {type(x).__name__}")
        if len(x) > _ffi.SPL_HEAL_MAX_PREFIX:
            raise ValueError(f"prefix {b} must have at most {_ffi.SPL_HEAL_MAX_PREFIX} bytes, not {len(x)}")
        rows[b, 0] = len(x)
        rows[b, 1:] = np.frombuffer(bytes(x) + b"\0" * (_ffi.SPL_HEAL_MAX_PREFIX - len(x)), dtype="<u8")
    return torch.from_numpy(rows.view(np.int64)).to(torch.device("cuda") if device is None else device)


def check_heal_args(ids, lengths=None, state=None, *, begin: bool, n_words=None, max_back: int = 0, min_keep: int = 0,
                    padding_side: str = "right", keep_free: bool = False, mask=None, state_out=None) -> None:
    """ValueError for a dtype, rank, shape, layout, size or device that heal_begin_device / heal_step_device would refuse -- before anything
    goes to the device."""
    left = _side("padding_side", padding_side)
    if not isinstance(ids, torch.Tensor) or ids.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"the ids must be a torch tensor of dtype int32 or int64, not {getattr(ids, 'dtype', type(ids))}")
    if ids.dim() not in ((2,) if begin else (1, 2)):
        raise ValueError("the prompts must have rank 2 ([batch, length])" if begin else "the ids must have rank 1 ([batch]) or 2 ([batch, steps])")
    if not ids.is_contiguous():
        raise ValueError("the ids must be contiguous")
    B = int(ids.shape[0])
    if B >= (1 << 31) or (ids.dim() == 2 and ids.shape[1] >= (1 << 32)):
        raise ValueError("the sequences must be fewer than 2**31 and a row shorter than 2**32")
    for name, v, top in (("max_back", max_back, _ffi.SPL_HEAL_MAX_BACK), ("min_keep", min_keep, (1 << 32) - 1)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= top:
            raise ValueError(f"{name} must be an integer in 0 .. {top}, not {v!r}")
    if n_words is not None and (isinstance(n_words, bool) or not isinstance(n_words, (int, np.integer)) or not 1 <= int(n_words) <= (1 << 26)):
        raise ValueError(f"n_words must be an integer in 1 .. 2**26, not {n_words!r}")
    others = []
    if lengths is not None:
        others.append(_vec("lengths", lengths, B, (torch.int32,), "int32"))
    elif left:
        raise ValueError("padding_side 'left' needs lengths")

    def rows(name, t):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.shape != (B, _ffi.SPL_HEAL_STATE_WORDS) or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous int64 tensor of shape [batch, {_ffi.SPL_HEAL_STATE_WORDS}]")
        others.append((name, t))

    if not begin:
        rows("state", state)
    if state_out is not None:
        rows("state_out", state_out)
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.dtype != torch.int32 or mask.dim() != 2 or mask.shape[0] != B or not mask.is_contiguous() or \
                (n_words is not None and mask.shape[1] != int(n_words)):
            raise ValueError("mask must be a contiguous int32 tensor of shape [batch, n_words]")
        others.append(("mask", mask))
    elif keep_free:
        raise ValueError("keep_free needs the caller's mask (its free rows filled with ones once)")
    if not ids.is_cuda:
        raise ValueError("the ids must be on a GPU (device-side token healing takes no host tensor)")
    for name, t in others:
        if t.device != ids.device:
            raise ValueError(f"{name} must be on the device of the ids")


def _heal_call(tok: Tokenizer, begin: bool, ids, lengths, state, flags: int, n_words, max_back: int, min_keep: int, mask, state_out):
    dev = ids.device
    B = int(ids.shape[0])
    K = int(ids.shape[1]) if ids.dim() == 2 else 1
    n_words = int(mask.shape[1]) if mask is not None else (heal_n_words(tok) if n_words is None else int(n_words))
    if mask is None:
        mask = torch.empty((B, n_words), dtype=torch.int32, device=dev)          # (every word of every row is written by the kernels)
    if state_out is None:
        state_out = torch.empty((B, _ffi.SPL_HEAL_STATE_WORDS), dtype=torch.int64, device=dev)
    live = torch.empty(max(B, 1), dtype=torch.uint8, device=dev)[:B]
    n = torch.empty(2, dtype=torch.int32, device=dev)
    n_back = torch.empty(max(B, 1), dtype=torch.int32, device=dev)[:B] if begin else None
    flags |= _ffi.SPL_HEAL_I64 if ids.dtype == torch.int64 else 0
    # (null state, mask and n_back pointers are refused by the library: an empty batch passes addresses of its own, which nothing dereferences)
    spare = torch.empty(8, dtype=torch.int64, device=dev).data_ptr() if B == 0 or n_words == 0 else 0
    si = _ffi.SplHealIn(B, K, _ptr(ids), _ptr(lengths), None if begin else (_ptr(state) or spare))
    o = _ffi.SplHealOpts(flags, n_words, max_back, min_keep)
    so = _ffi.SplHealOut(_ptr(state_out) or spare, _ptr(mask) or spare + 16, _ptr(live), n.data_ptr(), (_ptr(n_back) or spare + 32) if begin else None)
    L = _ffi.lib()
    fn, name = (L.spl_heal_begin_device, "spl_heal_begin_device") if begin else (L.spl_heal_step_device, "spl_heal_step_device")
    rc = fn(tok.handle, ctypes.byref(si), ctypes.byref(o), ctypes.byref(so), torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        _raise_rc(rc, name)
    return n_back, state_out, mask, live, n


def heal_begin_device(tok: Tokenizer, rows: torch.Tensor, lengths: Optional[torch.Tensor] = None, *, max_back: int = 1, min_keep: int = 0,
                      auto: bool = True, padding_side: str = "right", n_words: Optional[int] = None, keep_free: bool = False,
                      mask: Optional[torch.Tensor] = None, state_out: Optional[torch.Tensor] = None):
    """Token healing, the start (spl_heal_begin_device), on torch's current stream; nothing synchronises.  rows int32 / int64 [B, L]: the
    prompts, lengths int32 [B] (None: every entry), padding_side as decode_rows_device takes it.  Up to max_back (0 .. 8) tokens are taken
    off every prompt's end -- while at least min_keep remain, the token is an ordinary one, the bytes taken fit 64, and with auto only
    while some token extends what has been taken.  Returns (n_back int32 [B], state int64 [B, 9], mask int32 [B, n_words], live uint8 [B],
    n int32 [2]): feed the model the first lengths - n_back tokens and let it sample where mask has a 1 (bit t & 31 of word t >> 5: id t,
    the layout of xgrammar's apply_token_bitmask); n = (constrained sequences, 0).  n_words: default heal_n_words(tok), or mask's."""
    check_heal_args(rows, lengths, begin=True, n_words=n_words, max_back=max_back, min_keep=min_keep, padding_side=padding_side,
                    keep_free=keep_free, mask=mask, state_out=state_out)
    flags = (_ffi.SPL_HEAL_AUTO if auto else 0) | (_ffi.SPL_HEAL_PAD_LEFT if padding_side == "left" else 0) | \
        (_ffi.SPL_HEAL_KEEP_FREE if keep_free else 0)
    return _heal_call(tok, True, rows, lengths, None, flags, n_words, int(max_back), int(min_keep), mask, state_out)


def heal_step_device(tok: Tokenizer, ids: Optional[torch.Tensor], lengths: Optional[torch.Tensor], state: torch.Tensor, *,
                     n_words: Optional[int] = None, keep_free: bool = False, mask: Optional[torch.Tensor] = None,
                     state_out: Optional[torch.Tensor] = None):
    """Token healing, one step (spl_heal_step_device), on torch's current stream; nothing synchronises.  ids [B] or [B, K] int32 / int64:
    what the sampler drew (a sequence's first lengths[b] entries count, all with lengths None); None: no ids, the masks of the state rows
    as they are -- the first call after heal_state_from_prefixes.  A covering id heals a sequence, a partial one shortens its prefix,
    anything else breaks it (it runs free, `broken` set).  Returns (state_out int64 [B, 9], mask int32 [B, n_words], live uint8 [B],
    n int32 [2]: constrained sequences, sequences that broke in this call).  state_out may be state.  keep_free: rows of sequences that are
    free after the call are not written -- pass the mask whose free rows hold ones already."""
    if ids is None:
        if not isinstance(state, torch.Tensor) or state.dim() != 2:
            raise ValueError(f"state must be a contiguous int64 tensor of shape [batch, {_ffi.SPL_HEAL_STATE_WORDS}]")
        ids = torch.empty((state.shape[0], 0), dtype=torch.int32, device=state.device)
    check_heal_args(ids, lengths, state, begin=False, n_words=n_words, keep_free=keep_free, mask=mask, state_out=state_out)
    flags = _ffi.SPL_HEAL_KEEP_FREE if keep_free else 0
    return _heal_call(tok, False, ids, lengths, state, flags, n_words, 0, 0, mask, state_out)[1:]


class TokenHealer:
    """`tokenizer.token_healer(batch_size)`: token healing for a batch whose state lives on the GPU.  begin(rows, lengths) takes the last
    tokens off the prompts and returns how many; step(ids) follows the sampler; `mask` (int32 [B, n_words], the apply_token_bitmask layout)
    always holds the ids the next step may draw -- all ones for a sequence that is free.  Nothing here synchronises."""

    def __init__(self, tok: Tokenizer, batch_size: int, n_words: Optional[int] = None, max_back: int = 1, auto: bool = True):
        if isinstance(batch_size, bool) or not isinstance(batch_size, (int, np.integer)) or not 0 <= int(batch_size) < (1 << 31):
            raise ValueError(f"batch_size must be an integer in 0 .. 2**31 - 1, not {batch_size!r}")
        self._tok, self.batch_size, self.max_back, self.auto = tok, int(batch_size), max_back, bool(auto)
        self.n_words = heal_n_words(tok) if n_words is None else int(n_words)
        dev = torch.device("cuda", tok._device)
        self.mask = torch.full((self.batch_size, self.n_words), -1, dtype=torch.int32, device=dev)
        self._state = torch.zeros((self.batch_size, _ffi.SPL_HEAL_STATE_WORDS), dtype=torch.int64, device=dev)
        self.live = torch.zeros(self.batch_size, dtype=torch.uint8, device=dev)
        self.n = torch.zeros(2, dtype=torch.int32, device=dev)
        check_heal_args(torch.empty((self.batch_size, 0), dtype=torch.int32, device=dev), None, self._state, begin=False, n_words=self.n_words,
                        max_back=max_back)
        heal_reserve(tok, self.batch_size)

    def begin(self, rows: torch.Tensor, lengths: Optional[torch.Tensor] = None, *, padding_side: str = "right", min_keep: int = 0) -> torch.Tensor:
        """The prompts [B, L] -> n_back int32 [B] on the device; state, mask and live are this batch's from here on."""
        n_back, _, _, self.live, self.n = heal_begin_device(self._tok, rows, lengths, max_back=self.max_back, min_keep=min_keep, auto=self.auto,
                                                            padding_side=padding_side, mask=self.mask, state_out=self._state)
        return n_back

    def step(self, ids: Optional[torch.Tensor], lengths: Optional[torch.Tensor] = None, *, keep_free: bool = False) -> torch.Tensor:
        """What the sampler drew, [B] or [B, K] (None: only the masks, after the caller wrote prefixes into `state`) -> the mask.
        keep_free: the rows of free sequences are not written again -- right once a step WITHOUT it has run after the last sequence
        left its constraint (its row holds ones since then)."""
        _, _, self.live, self.n = heal_step_device(self._tok, ids, lengths, self._state, keep_free=keep_free, mask=self.mask, state_out=self._state)
        return self.mask

    def reset(self, rows=None) -> None:
        """All sequences (rows None) or the given ones (indices or a bool mask) free and fresh, their mask rows ones."""
        if rows is None:
            self._state.zero_(); self.mask.fill_(-1); self.live.zero_()
        else:
            self._state[rows] = 0
            self.mask[rows] = -1
            self.live[rows] = 0

    def apply(self, logits: torch.Tensor, *, live_only: bool = False) -> torch.Tensor:
        """logits [B, V] (float32, float16 or bfloat16) with -inf wherever the mask forbids the id, IN PLACE: one launch of
        mask_apply_device.  Columns beyond 32 * n_words are left as they are.  live_only: the rows of free sequences (`live` 0) are
        skipped -- their mask rows hold ones, so the result is the same and such a row costs one byte."""
        if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.shape[0] != self.batch_size:
            raise ValueError("logits must have shape [batch, vocabulary]")
        return mask_apply_device(self._tok, logits, self.mask, live=self.live if live_only else None)

    @property
    def state(self) -> torch.Tensor:
        """int64 [B, 9] on the device, as include/splintr_hip.h lays it out (the healer's own tensor: a prefix written here counts)"""
        return self._state

    @property
    def pending(self) -> torch.Tensor:
        """int64 [B] on the device: the bytes of every sequence's pending prefix"""
        return self._state[:, 0] & 0x7F

    @property
    def broken(self) -> torch.Tensor:
        return ((self._state[:, 0] >> 8) & 1).bool()

    @property
    def healed(self) -> torch.Tensor:
        return ((self._state[:, 0] >> 9) & 1).bool()

    def __repr__(self) -> str:
        return f"TokenHealer(batch_size={self.batch_size}, n_words={self.n_words}, max_back={self.max_back}, auto={self.auto})"


# ---------------------------------------------------------------------------------------------- UTF-8 continuation masks, bitmask -> logits
def utf8_mask_reserve(tok: Tokenizer) -> None:
    """spl_utf8_mask_reserve_device: the decode tables on the device and, built there, the table of the eight UTF-8 classes (again after
    spl_add_special); utf8_mask_device calls then neither allocate nor synchronise."""
    rc = _ffi.lib().spl_utf8_mask_reserve_device(tok.handle)
    if rc != 0:
        _raise_rc(rc, "spl_utf8_mask_reserve_device")


def check_utf8_mask_args(state, *, n_words=None, out=None, and_into: bool = False) -> None:
    """ValueError for a dtype, rank, shape, layout or device that utf8_mask_device would refuse -- before anything goes to the device."""
    if not isinstance(state, torch.Tensor) or state.dtype != torch.int64 or state.dim() != 1 or not state.is_contiguous():
        raise ValueError("state must be a contiguous int64 tensor of shape [batch] (the streaming decode's state words)")
    if state.shape[0] >= (1 << 31):
        raise ValueError("the sequences must be fewer than 2**31")
    if n_words is not None and (isinstance(n_words, bool) or not isinstance(n_words, (int, np.integer)) or not 1 <= int(n_words) <= (1 << 26)):
        raise ValueError(f"n_words must be an integer in 1 .. 2**26, not {n_words!r}")
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.int32 or out.dim() != 2 or out.shape[0] != state.shape[0] or \
                not out.is_contiguous() or not 1 <= out.shape[1] <= (1 << 26) or (n_words is not None and out.shape[1] != int(n_words)):
            raise ValueError("out must be a contiguous int32 tensor of shape [batch, n_words]")
    elif and_into:
        raise ValueError("and_into needs out (the mask the rows are ANDed into)")
    if not state.is_cuda:
        raise ValueError("state must be on a GPU (the device-side UTF-8 mask takes no host tensor)")
    if out is not None and out.device != state.device:
        raise ValueError("out must be on the device of state")


def utf8_mask_device(tok: Tokenizer, state: torch.Tensor, *, n_words: Optional[int] = None, skip_special_tokens: bool = False,
                     out: Optional[torch.Tensor] = None, and_into: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """UTF-8 continuation masks (spl_utf8_mask_device), on torch's current stream; nothing synchronises.  state int64 [B]: the streaming
    decode's state words.  Returns (mask int32 [B, n_words], live uint8 [B]): bit t & 31 of word t >> 5 is 1 iff id t is known and its
    bytes (none for a special id with skip_special_tokens) keep the sequence's text well-formed UTF-8 behind what is pending; a stalled
    sequence has a row of ones and live 0.  out: the mask to write; and_into: the rows are ANDed into it.  n_words: default
    heal_n_words(tok), or out's."""
    check_utf8_mask_args(state, n_words=n_words, out=out, and_into=and_into)
    dev = state.device
    B = int(state.shape[0])
    n_words = int(out.shape[1]) if out is not None else (heal_n_words(tok) if n_words is None else int(n_words))
    if out is None:
        out = torch.empty((B, n_words), dtype=torch.int32, device=dev)            # (every word of every row is written by the kernel)
    live = torch.empty(max(B, 1), dtype=torch.uint8, device=dev)[:B]
    # (null state and mask pointers are refused by the library: an empty batch passes addresses of its own, which nothing dereferences)
    spare = torch.empty(4, dtype=torch.int64, device=dev).data_ptr() if B == 0 else 0
    o = _ffi.SplDecodeOpts(_ffi.SPL_DECODE_SKIP_SPECIAL if skip_special_tokens else 0, 1)
    rc = _ffi.lib().spl_utf8_mask_device(tok.handle, _ptr(state) or spare, B, ctypes.byref(o), _ffi.SPL_UTF8_AND if and_into else 0, n_words,
                                         _ptr(out) or spare + 16, _ptr(live), torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        _raise_rc(rc, "spl_utf8_mask_device")
    return out, live


_MASK_DTYPES = {torch.float32: _ffi.SPL_F32, torch.float16: _ffi.SPL_F16, torch.bfloat16: _ffi.SPL_BF16}


def check_mask_apply_args(logits, mask, *, live=None) -> None:
    """ValueError for a dtype, rank, shape, layout or device that mask_apply_device would refuse -- before anything goes to the device."""
    if not isinstance(logits, torch.Tensor) or logits.dtype not in _MASK_DTYPES:
        raise ValueError(f"logits must be a torch tensor of dtype float32, float16 or bfloat16, not {getattr(logits, 'dtype', type(logits))}")
    if logits.dim() != 2:
        raise ValueError(f"logits must have rank 2 ([batch, vocabulary]), not {logits.dim()}")
    R, C = int(logits.shape[0]), int(logits.shape[1])
    if R >= (1 << 31) or C >= (1 << 32):
        raise ValueError("the rows must be fewer than 2**31 and the columns fewer than 2**32")
    if R and C > 1 and logits.stride(1) != 1 or R > 1 and C and logits.stride(0) < C:
        raise ValueError("a row of the logits must be contiguous and the rows must not overlap (stride(1) == 1, stride(0) >= columns)")
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.int32 or mask.dim() != 2 or mask.shape[0] != R:
        raise ValueError("mask must be an int32 tensor of shape [batch, n_words]")
    W = int(mask.shape[1])
    if W > (1 << 26):
        raise ValueError("mask must have at most 2**26 words a row")
    if R and W > 1 and mask.stride(1) != 1 or R > 1 and W and mask.stride(0) < W:
        raise ValueError("a row of the mask must be contiguous and the rows must not overlap (stride(1) == 1, stride(0) >= n_words)")
    if live is not None:
        _vec("live", live, R, (torch.uint8, torch.bool), "uint8 or bool")
    if not logits.is_cuda:
        raise ValueError("logits must be on a GPU (the device-side mask apply takes no host tensor)")
    for name, t in (("mask", mask), ("live", live)):
        if t is not None and t.device != logits.device:
            raise ValueError(f"{name} must be on the device of the logits")


def mask_apply_device(tok: Tokenizer, logits: torch.Tensor, mask: torch.Tensor, *, live: Optional[torch.Tensor] = None) -> torch.Tensor:
    """An allowed-token bitmask applied to the logits IN PLACE (spl_mask_apply_device), on torch's current stream; nothing synchronises.
    logits [B, V] float32 / float16 / bfloat16 -- any view whose rows are contiguous (a sliced base and an odd row width are fine); mask
    int32 [B, n_words], bit t & 31 of word t >> 5 for column t (heal_*_device's, utf8_mask_device's and xgrammar's layout); live uint8 /
    bool [B]: rows with 0 are skipped, their mask rows not read.  Where a live row's bit is 0 the logit becomes -inf (a NaN too); every
    other element keeps its bits, columns at or beyond 32 * n_words included.  Returns logits."""
    check_mask_apply_args(logits, mask, live=live)
    R, C, W = int(logits.shape[0]), int(logits.shape[1]), int(mask.shape[1])
    a = _ffi.SplMaskApply(_MASK_DTYPES[logits.dtype], _ptr(logits), R, C, W, max(int(logits.stride(0)), C) if R > 1 else C,
                          max(int(mask.stride(0)), W) if R > 1 else W, _ptr(mask), _ptr(live))
    rc = _ffi.lib().spl_mask_apply_device(tok.handle, ctypes.byref(a), torch.cuda.current_stream(logits.device).cuda_stream)
    if rc != 0:
        _raise_rc(rc, "spl_mask_apply_device")
    return logits


# ---------------------------------------------------------------------------------------------- guided choice (masks for one-of-N answers)
def _choice_table_host(choices) -> np.ndarray:
    if isinstance(choices, (str, bytes, bytearray)) or not hasattr(choices, "__iter__"):
        raise ValueError("choices must be a list of str or bytes")
    choices = list(choices)
    if len(choices) > _ffi.SPL_CHOICE_SLOTS:
        raise ValueError(f"at most {_ffi.SPL_CHOICE_SLOTS} choices fit the table, not {len(choices)}")
    tab = np.zeros(_ffi.SPL_CHOICE_TABLE_BYTES, dtype=np.uint8)
    for s, x in enumerate(choices):
        if isinstance(x, str):
            x = x.encode("utf-8")
        elif not isinstance(x, (bytes, bytearray)):
            raise ValueError(f"choice {s} must be str or bytes, not {type(x).__name__}")
        if not 1 <= len(x) <= _ffi.SPL_CHOICE_MAX_LEN:
            raise ValueError(f"choice {s} must have 1 .. {_ffi.SPL_CHOICE_MAX_LEN} bytes, not {len(x)}")
        tab[_ffi.SPL_CHOICE_MAX_LEN * s:_ffi.SPL_CHOICE_MAX_LEN * s + len(x)] = np.frombuffer(bytes(x), dtype=np.uint8)
        tab[_ffi.SPL_CHOICE_SLOTS * _ffi.SPL_CHOICE_MAX_LEN + s] = len(x)
    return tab


def choice_table(choices, device=None) -> torch.Tensor:
    """The choice table of spl_choice_step_device on the device (default: the current GPU): uint8 [4160], slot s = choices[s] (str: its
    UTF-8).  ValueError for an empty choice, one over 64 bytes, or more than 64 choices.  The tensor is the caller's."""
    tab = _choice_table_host(choices)
    return torch.from_numpy(tab).to(torch.device("cuda") if device is None else device)


def _choice_state_host(selections, n_choices: int) -> np.ndarray:
    if isinstance(n_choices, bool) or not isinstance(n_choices, (int, np.integer)) or not 0 <= int(n_choices) <= _ffi.SPL_CHOICE_SLOTS:
        raise ValueError(f"n_choices must be an integer in 0 .. {_ffi.SPL_CHOICE_SLOTS}, not {n_choices!r}")
    if isinstance(selections, (str, bytes, bytearray)) or not hasattr(selections, "__iter__"):
        raise ValueError("selections must be a list with None or an iterable of slot indices per sequence")
    selections = list(selections)
    rows = np.zeros((len(selections), _ffi.SPL_CHOICE_STATE_WORDS), dtype=np.uint64)
    every = (1 << int(n_choices)) - 1
    for b, sel in enumerate(selections):
        if sel is None:
            rows[b, 0] = every
            continue
        if isinstance(sel, (str, bytes, bytearray)) or not hasattr(sel, "__iter__"):
            raise ValueError(f"selection {b} must be None or an iterable of slot indices")
        w = 0
        for s in sel:
            if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or not 0 <= int(s) < int(n_choices):
                raise ValueError(f"selection {b} names slot {s!r}: slots are 0 .. {int(n_choices) - 1}")
            w |= 1 << int(s)
        rows[b, 0] = w
    return rows


def choice_state(selections, n_choices: int, device=None) -> torch.Tensor:
    """State rows int64 [len(selections), 2] for sequences that begin: per sequence None (every slot below n_choices) or an iterable of slot
    indices (an empty one: a free row), built on the host -- choice_step_device with ids None then writes the first masks.  The tensor
    goes to `device` (default: the current GPU)."""
    rows = _choice_state_host(selections, n_choices)
    return torch.from_numpy(rows.view(np.int64)).to(torch.device("cuda") if device is None else device)


def choice_n_words(tok: Tokenizer) -> int:
    """The words of a mask row that cover every id the tokenizer knows (specials included)."""
    return heal_n_words(tok)


def choice_reserve(tok: Tokenizer) -> None:
    """spl_choice_reserve_device: the decode tables and token healing's sorted order and prefix order on the device (shared with
    heal_reserve); choice_step_device calls then neither allocate nor synchronise."""
    rc = _ffi.lib().spl_choice_reserve_device(tok.handle)
    if rc != 0:
        _raise_rc(rc, "spl_choice_reserve_device")


def _choice_end_ids(end_ids, then_free: bool, n_words=None):
    end_ids = [] if end_ids is None else ([end_ids] if isinstance(end_ids, (int, np.integer)) and not isinstance(end_ids, bool) else list(end_ids))
    for e in end_ids:
        if isinstance(e, bool) or not isinstance(e, (int, np.integer)) or not 0 <= int(e) < (1 << 32):
            raise ValueError(f"an END id must be an integer in 0 .. 2**32 - 1, not {e!r}")
        if n_words is not None and int(e) >= 32 * int(n_words):
            raise ValueError(f"END id {int(e)} is at or above 32 * n_words")
    if len(end_ids) > _ffi.SPL_CHOICE_MAX_END:
        raise ValueError(f"at most {_ffi.SPL_CHOICE_MAX_END} END ids, not {len(end_ids)}")
    if not end_ids and not then_free:
        raise ValueError("end_ids is empty and then_free is not set: no sequence could ever finish")
    return [int(e) for e in end_ids]


def check_choice_args(ids, lengths, state, table, *, end_ids=None, then_free: bool = False, n_words=None, keep_free: bool = False, mask=None,
                      state_out=None) -> None:
    """ValueError for a dtype, rank, shape, layout, size or device that choice_step_device would refuse -- before anything goes to the
    device."""
    if not isinstance(ids, torch.Tensor) or ids.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"the ids must be a torch tensor of dtype int32 or int64, not {getattr(ids, 'dtype', type(ids))}")
    if ids.dim() not in (1, 2):
        raise ValueError("the ids must have rank 1 ([batch]) or 2 ([batch, steps])")
    if not ids.is_contiguous():
        raise ValueError("the ids must be contiguous")
    B = int(ids.shape[0])
    if B >= (1 << 31) or (ids.dim() == 2 and ids.shape[1] >= (1 << 32)):
        raise ValueError("the sequences must be fewer than 2**31 and a row shorter than 2**32")
    if n_words is not None and (isinstance(n_words, bool) or not isinstance(n_words, (int, np.integer)) or not 1 <= int(n_words) <= (1 << 26)):
        raise ValueError(f"n_words must be an integer in 1 .. 2**26, not {n_words!r}")
    if not isinstance(table, torch.Tensor) or table.dtype != torch.uint8 or table.shape != (_ffi.SPL_CHOICE_TABLE_BYTES,) or not table.is_contiguous():
        raise ValueError(f"table must be a contiguous uint8 tensor of shape [{_ffi.SPL_CHOICE_TABLE_BYTES}] (choice_table)")
    others = [("table", table)]
    if lengths is not None:
        others.append(_vec("lengths", lengths, B, (torch.int32,), "int32"))

    def rows(name, t):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.shape != (B, _ffi.SPL_CHOICE_STATE_WORDS) or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous int64 tensor of shape [batch, {_ffi.SPL_CHOICE_STATE_WORDS}]")
        others.append((name, t))

    rows("state", state)
    if state_out is not None:
        rows("state_out", state_out)
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.dtype != torch.int32 or mask.dim() != 2 or mask.shape[0] != B or not mask.is_contiguous() or \
                (n_words is not None and mask.shape[1] != int(n_words)):
            raise ValueError("mask must be a contiguous int32 tensor of shape [batch, n_words]")
        others.append(("mask", mask))
    elif keep_free:
        raise ValueError("keep_free needs the caller's mask (the rows of sequences that are not constrained filled with ones once)")
    _choice_end_ids(end_ids, then_free, int(mask.shape[1]) if mask is not None else n_words)
    if not ids.is_cuda:
        raise ValueError("the ids must be on a GPU (device-side guided choice takes no host tensor)")
    for name, t in others:
        if t.device != ids.device:
            raise ValueError(f"{name} must be on the device of the ids")


def choice_step_device(tok: Tokenizer, ids: Optional[torch.Tensor], lengths: Optional[torch.Tensor], state: torch.Tensor, table: torch.Tensor, *,
                       end_ids=None, then_free: bool = False, n_words: Optional[int] = None, keep_free: bool = False,
                       mask: Optional[torch.Tensor] = None, state_out: Optional[torch.Tensor] = None):
    """Guided choice, one step (spl_choice_step_device), on torch's current stream; nothing synchronises.  state int64 [B, 2]: the rows
    as include/splintr_hip.h lays them out (choice_state: the candidate sets of sequences that begin); table: choice_table(...); ids [B]
    or [B, K] int32 / int64: what the sampler drew (a sequence's first lengths[b] entries count, all with lengths None); None: no ids, the
    masks of the state rows as they are -- the first call after choice_state.  An id some remaining choice goes on with narrows the
    candidates; an END id (end_ids: up to 8 ids, usually specials) behind a choice that is spelled out ends the sequence (`done`, with
    `hit` the slot); with then_free a sequence is done as soon as a choice is spelled out and END ids play no part; anything else breaks
    it (it runs free, `broken` set).  Returns (state_out int64 [B, 2], mask int32 [B, n_words], live uint8 [B]: 1 where the sequence is
    constrained after the call).  state_out may be state.  keep_free: rows of sequences that are not constrained after the call are not
    written -- pass the mask whose rows hold ones for them already.  n_words: default choice_n_words(tok), or mask's."""
    if ids is None:
        if not isinstance(state, torch.Tensor) or state.dim() != 2:
            raise ValueError(f"state must be a contiguous int64 tensor of shape [batch, {_ffi.SPL_CHOICE_STATE_WORDS}]")
        ids = torch.empty((state.shape[0], 0), dtype=torch.int32, device=state.device)
    check_choice_args(ids, lengths, state, table, end_ids=end_ids, then_free=then_free, n_words=n_words, keep_free=keep_free, mask=mask,
                      state_out=state_out)
    dev = ids.device
    B = int(ids.shape[0])
    K = int(ids.shape[1]) if ids.dim() == 2 else 1
    n_words = int(mask.shape[1]) if mask is not None else (choice_n_words(tok) if n_words is None else int(n_words))
    ends = _choice_end_ids(end_ids, then_free, n_words)
    if mask is None:
        mask = torch.empty((B, n_words), dtype=torch.int32, device=dev)          # (every word of every row is written by the kernel)
    if state_out is None:
        state_out = torch.empty((B, _ffi.SPL_CHOICE_STATE_WORDS), dtype=torch.int64, device=dev)
    live = torch.empty(max(B, 1), dtype=torch.uint8, device=dev)[:B]
    flags = (_ffi.SPL_CHOICE_THEN_FREE if then_free else 0) | (_ffi.SPL_CHOICE_KEEP_FREE if keep_free else 0) | \
        (_ffi.SPL_CHOICE_I64 if ids.dtype == torch.int64 else 0)
    # (null state and mask pointers are refused by the library: an empty batch passes addresses of its own, which nothing dereferences)
    spare = torch.empty(8, dtype=torch.int64, device=dev).data_ptr() if B == 0 else 0
    si = _ffi.SplChoiceIn(B, K, _ptr(ids), _ptr(lengths), _ptr(state) or spare, _ptr(table))
    o = _ffi.SplChoiceOpts(flags, n_words, ends)
    so = _ffi.SplChoiceOut(_ptr(state_out) or spare + 16, _ptr(mask) or spare + 32, _ptr(live))
    rc = _ffi.lib().spl_choice_step_device(tok.handle, ctypes.byref(si), ctypes.byref(o), ctypes.byref(so), torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        _raise_rc(rc, "spl_choice_step_device")
    return state_out, mask, live


class ChoiceGuide:
    """`tokenizer.choice_guide(batch_size, choices)`: "the answer is exactly one of these strings" for a batch whose state lives on the
    GPU.  begin(selections) writes the candidate sets and the first masks; step(ids) follows the sampler; `mask` (int32 [B, n_words], the
    apply_token_bitmask layout) always holds the ids the next step may draw -- all ones for a sequence that is free, done or broken.
    Nothing here synchronises."""

    def __init__(self, tok: Tokenizer, batch_size: int, choices, *, end_ids=None, then_free: bool = False, n_words: Optional[int] = None):
        if isinstance(batch_size, bool) or not isinstance(batch_size, (int, np.integer)) or not 0 <= int(batch_size) < (1 << 31):
            raise ValueError(f"batch_size must be an integer in 0 .. 2**31 - 1, not {batch_size!r}")
        self._tok, self.batch_size, self.then_free = tok, int(batch_size), bool(then_free)
        self.n_words = choice_n_words(tok) if n_words is None else int(n_words)
        if not isinstance(choices, (str, bytes, bytearray)) and hasattr(choices, "__iter__"):
            choices = list(choices)
        tab = _choice_table_host(choices)
        self.n_choices = len(choices)
        self.end_ids = _choice_end_ids(end_ids, self.then_free, self.n_words)
        dev = torch.device("cuda", tok._device)
        self.table = torch.from_numpy(tab).to(dev)
        self.mask = torch.full((self.batch_size, self.n_words), -1, dtype=torch.int32, device=dev)
        self._state = torch.zeros((self.batch_size, _ffi.SPL_CHOICE_STATE_WORDS), dtype=torch.int64, device=dev)
        self.live = torch.zeros(self.batch_size, dtype=torch.uint8, device=dev)
        check_choice_args(torch.empty((self.batch_size, 0), dtype=torch.int32, device=dev), None, self._state, self.table, end_ids=self.end_ids,
                          then_free=self.then_free, n_words=self.n_words)
        choice_reserve(tok)

    def _call(self, ids, lengths, keep_free):
        _, _, self.live = choice_step_device(self._tok, ids, lengths, self._state, self.table, end_ids=self.end_ids, then_free=self.then_free,
                                             keep_free=keep_free, mask=self.mask, state_out=self._state)
        return self.mask

    def begin(self, selections=None, rows=None) -> torch.Tensor:
        """The candidate sets of sequences that begin, and the first masks -> the mask.  selections: None (every sequence: every choice), or
        per sequence None or an iterable of slot indices (an empty one: the sequence runs free).  rows: the sequences that begin (indices or
        a bool mask; selections then has one entry per such sequence); the others keep their state."""
        dev = self._state.device
        if rows is None:
            sel = [None] * self.batch_size if selections is None else list(selections)
            if len(sel) != self.batch_size:
                raise ValueError(f"selections must have one entry per sequence ({self.batch_size}), not {len(sel)}")
            self._state.copy_(torch.from_numpy(_choice_state_host(sel, self.n_choices).view(np.int64)).to(dev), non_blocking=True)
        else:
            idx = torch.as_tensor(rows, device=dev)
            idx = idx.nonzero().flatten() if idx.dtype == torch.bool else idx.to(torch.int64).flatten()
            sel = [None] * int(idx.numel()) if selections is None else list(selections)
            if len(sel) != int(idx.numel()):
                raise ValueError(f"selections must have one entry per row that begins ({int(idx.numel())}), not {len(sel)}")
            self._state[idx] = torch.from_numpy(_choice_state_host(sel, self.n_choices).view(np.int64)).to(dev)
        return self._call(None, None, False)

    def step(self, ids: Optional[torch.Tensor], lengths: Optional[torch.Tensor] = None, *, keep_free: bool = False) -> torch.Tensor:
        """What the sampler drew, [B] or [B, K] (None: only the masks, after the caller wrote rows into `state`) -> the mask.  keep_free:
        the rows of sequences that are not constrained are not written again -- right once a step WITHOUT it has run after the last
        sequence left its constraint (its row holds ones since then)."""
        return self._call(ids, lengths, keep_free)

    def reset(self, rows=None) -> None:
        """All sequences (rows None) or the given ones (indices or a bool mask) free and fresh, their mask rows ones."""
        if rows is None:
            self._state.zero_(); self.mask.fill_(-1); self.live.zero_()
        else:
            self._state[rows] = 0
            self.mask[rows] = -1
            self.live[rows] = 0

    def apply(self, logits: torch.Tensor, *, live_only: bool = False) -> torch.Tensor:
        """logits [B, V] (float32, float16 or bfloat16) with -inf wherever the mask forbids the id, IN PLACE: one launch of
        mask_apply_device.  live_only: the rows of sequences that are not constrained (`live` 0) are skipped -- their mask rows hold ones,
        so the result is the same."""
        if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.shape[0] != self.batch_size:
            raise ValueError("logits must have shape [batch, vocabulary]")
        return mask_apply_device(self._tok, logits, self.mask, live=self.live if live_only else None)

    @property
    def state(self) -> torch.Tensor:
        """int64 [B, 2] on the device, as include/splintr_hip.h lays it out (the guide's own tensor: a row written here counts)"""
        return self._state

    @property
    def spelled(self) -> torch.Tensor:
        """int64 [B] on the device: k, the bytes every sequence has spelled so far"""
        return self._state[:, 1] & 0x7F

    @property
    def broken(self) -> torch.Tensor:
        return ((self._state[:, 1] >> 8) & 1).bool()

    @property
    def done(self) -> torch.Tensor:
        return ((self._state[:, 1] >> 9) & 1).bool()

    @property
    def hit(self) -> torch.Tensor:
        """int64 [B] on the device: the slot a done sequence answered, -1 for every other sequence"""
        w = self._state[:, 1]
        return torch.where((w >> 9) & 1 != 0, (w >> 16) & 63, torch.full_like(w, -1))

    def __repr__(self) -> str:
        return f"ChoiceGuide(batch_size={self.batch_size}, n_choices={self.n_choices}, n_words={self.n_words}, then_free={self.then_free})"


# ---------------------------------------------------------------------------------------------- the regex guide (masks from a byte DFA)
def _dfa_of(dfa):
    """(trans uint16 [S, 256], accept uint8 [S]) of a splintr_amd.dfa.ByteDFA or of such a pair, checked."""
    trans, accept = (dfa.trans, dfa.accept) if hasattr(dfa, "trans") else dfa
    trans, accept = np.asarray(trans), np.asarray(accept)
    if trans.dtype != np.uint16 or trans.ndim != 2 or trans.shape[1] != 256 or not 1 <= trans.shape[0] <= _ffi.SPL_DFA_MAX_STATES:
        raise ValueError(f"the transitions must be a uint16 array of shape [n_states, 256] with n_states in 1 .. {_ffi.SPL_DFA_MAX_STATES}")
    if accept.shape != (trans.shape[0],):
        raise ValueError("accept must have one entry per state")
    return trans, (accept != 0).astype(np.uint8)


def _dfa_table_host(dfa) -> np.ndarray:
    trans, accept = _dfa_of(dfa)
    return np.concatenate([np.ascontiguousarray(trans, dtype="<u2").view(np.uint8).reshape(-1), accept])


def dfa_table(dfa, device=None) -> torch.Tensor:
    """The DFA table of spl_dfa_index_device / spl_dfa_step_device on the device (default: the current GPU): uint8 [S * 512 + S] -- uint16
    trans[S][256], then accept[S].  dfa: a splintr_amd.dfa.ByteDFA (compile_regex, stack) or (trans, accept).  The tensor is the caller's."""
    return torch.from_numpy(_dfa_table_host(dfa)).to(torch.device("cuda") if device is None else device)


def _dfa_state_host(starts) -> np.ndarray:
    if isinstance(starts, (str, bytes, bytearray)) or not hasattr(starts, "__iter__"):
        raise ValueError("starts must be a list with None or a start state per sequence")
    rows = []
    for b, q in enumerate(starts):
        if q is None:
            rows.append(0)
            continue
        if isinstance(q, bool) or not isinstance(q, (int, np.integer)) or not 0 <= int(q) < _ffi.SPL_DFA_MAX_STATES:
            raise ValueError(f"start {b} must be None or a state in 0 .. {_ffi.SPL_DFA_MAX_STATES - 1}, not {q!r}")
        rows.append(int(q) | 1 << 16)
    return np.array(rows, dtype=np.int64).reshape(len(rows))


def dfa_state(starts, device=None) -> torch.Tensor:
    """State words int64 [len(starts)] for sequences that begin: per sequence a start state (start | 1 << 16) or None (a free row), built
    on the host -- dfa_step_device with ids None then writes the first masks.  The tensor goes to `device` (default: the current GPU)."""
    return torch.from_numpy(_dfa_state_host(starts)).to(torch.device("cuda") if device is None else device)


def dfa_n_words(tok: Tokenizer) -> int:
    """The words of a mask row that cover every id the tokenizer knows (specials included)."""
    return heal_n_words(tok)


def dfa_reserve(tok: Tokenizer) -> None:
    """spl_dfa_reserve_device: the decode tables and token healing's id -> rank on the device (shared with heal_reserve and
    choice_reserve); dfa_index_device and dfa_step_device calls then neither allocate nor synchronise."""
    rc = _ffi.lib().spl_dfa_reserve_device(tok.handle)
    if rc != 0:
        _raise_rc(rc, "spl_dfa_reserve_device")


def _dfa_end_ids(end_ids, n_words=None):
    end_ids = [] if end_ids is None else ([end_ids] if isinstance(end_ids, (int, np.integer)) and not isinstance(end_ids, bool) else list(end_ids))
    for e in end_ids:
        if isinstance(e, bool) or not isinstance(e, (int, np.integer)) or not 0 <= int(e) < (1 << 32):
            raise ValueError(f"an END id must be an integer in 0 .. 2**32 - 1, not {e!r}")
        if n_words is not None and int(e) >= 32 * int(n_words):
            raise ValueError(f"END id {int(e)} is at or above 32 * n_words")
    if not 1 <= len(end_ids) <= _ffi.SPL_DFA_MAX_END:
        raise ValueError(f"1 .. {_ffi.SPL_DFA_MAX_END} END ids are needed (without one no sequence could ever finish), not {len(end_ids)}")
    return [int(e) for e in end_ids]


def _dfa_check_table(table, n_states):
    if isinstance(n_states, bool) or not isinstance(n_states, (int, np.integer)) or not 1 <= int(n_states) <= _ffi.SPL_DFA_MAX_STATES:
        raise ValueError(f"n_states must be an integer in 1 .. {_ffi.SPL_DFA_MAX_STATES}, not {n_states!r}")
    if not isinstance(table, torch.Tensor) or table.dtype != torch.uint8 or table.shape != (_ffi.SPL_DFA_TABLE_BYTES(int(n_states)),) or \
            not table.is_contiguous():
        raise ValueError(f"table must be a contiguous uint8 tensor of shape [{_ffi.SPL_DFA_TABLE_BYTES(int(n_states))}] (dfa_table) for {int(n_states)} states")


def _dfa_check_n_words(n_words):
    if n_words is not None and (isinstance(n_words, bool) or not isinstance(n_words, (int, np.integer)) or not 1 <= int(n_words) <= (1 << 26)):
        raise ValueError(f"n_words must be an integer in 1 .. 2**26, not {n_words!r}")


def check_dfa_args(ids, lengths, state, table, index, n_states, *, end_ids=None, n_words=None, keep_free: bool = False, mask=None, state_out=None) -> None:
    """ValueError for a dtype, rank, shape, layout, size or device that dfa_step_device would refuse -- before anything goes to the device.
    n_words (or mask's width) must be the one the index was built with: the index's size is checked against it."""
    if not isinstance(ids, torch.Tensor) or ids.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"the ids must be a torch tensor of dtype int32 or int64, not {getattr(ids, 'dtype', type(ids))}")
    if ids.dim() not in (1, 2):
        raise ValueError("the ids must have rank 1 ([batch]) or 2 ([batch, steps])")
    if not ids.is_contiguous():
        raise ValueError("the ids must be contiguous")
    B = int(ids.shape[0])
    if B >= (1 << 31) or (ids.dim() == 2 and ids.shape[1] >= (1 << 32)):
        raise ValueError("the sequences must be fewer than 2**31 and a row shorter than 2**32")
    _dfa_check_n_words(n_words)
    _dfa_check_table(table, n_states)
    others = [("table", table)]
    if lengths is not None:
        others.append(_vec("lengths", lengths, B, (torch.int32,), "int32"))
    others.append(_vec("state", state, B, (torch.int64,), "int64"))
    if state_out is not None:
        others.append(_vec("state_out", state_out, B, (torch.int64,), "int64"))
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.dtype != torch.int32 or mask.dim() != 2 or mask.shape[0] != B or not mask.is_contiguous() or \
                (n_words is not None and mask.shape[1] != int(n_words)):
            raise ValueError("mask must be a contiguous int32 tensor of shape [batch, n_words]")
        others.append(("mask", mask))
    elif keep_free:
        raise ValueError("keep_free needs the caller's mask (the rows of sequences that are not constrained filled with ones once)")
    width = int(mask.shape[1]) if mask is not None else n_words
    if width is not None:
        want = _ffi.SPL_DFA_INDEX_BYTES(int(n_states), int(width))
        if not isinstance(index, torch.Tensor) or index.dtype != torch.uint8 or index.shape != (want,) or not index.is_contiguous():
            raise ValueError(f"index must be a contiguous uint8 tensor of shape [{want}] (dfa_index_device with the same n_states and n_words)")
    elif not isinstance(index, torch.Tensor) or index.dtype != torch.uint8 or index.dim() != 1 or not index.is_contiguous():
        raise ValueError("index must be a contiguous uint8 tensor (dfa_index_device)")
    others.append(("index", index))
    _dfa_end_ids(end_ids, width)
    if not ids.is_cuda:
        raise ValueError("the ids must be on a GPU (the device-side regex guide takes no host tensor)")
    for name, t in others:
        if t.device != ids.device:
            raise ValueError(f"{name} must be on the device of the ids")


def dfa_index_device(tok: Tokenizer, table: torch.Tensor, n_states: int, *, n_words: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The state x vocabulary index of a DFA table (spl_dfa_index_device), built on the GPU on torch's current stream; nothing
    synchronises.  Returns uint8 [n_states * (stride * 4 + 1)], stride = n_words rounded up to four: int32 rows[n_states][stride] -- bit
    t of row q is 1 iff id t is ordinary and its bytes can be walked from state q without dying -- then some[n_states].  dfa_index_rows
    gives the two views.  n_words: default dfa_n_words(tok).  Build it again after add_special_tokens."""
    _dfa_check_table(table, n_states)
    _dfa_check_n_words(n_words)
    if not table.is_cuda:
        raise ValueError("table must be on a GPU (dfa_table)")
    n_words = dfa_n_words(tok) if n_words is None else int(n_words)
    want = _ffi.SPL_DFA_INDEX_BYTES(int(n_states), n_words)
    if out is None:
        out = torch.empty(want, dtype=torch.uint8, device=table.device)           # (every word and every byte is written by the kernels)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.shape != (want,) or not out.is_contiguous() or out.device != table.device:
        raise ValueError(f"out must be a contiguous uint8 tensor of shape [{want}] on the device of the table")
    rc = _ffi.lib().spl_dfa_index_device(tok.handle, _ptr(table), int(n_states), n_words, _ptr(out), torch.cuda.current_stream(table.device).cuda_stream)
    if rc != 0:
        _raise_rc(rc, "spl_dfa_index_device")
    return out


def dfa_index_rows(index: torch.Tensor, n_states: int, n_words: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(rows int32 [n_states, stride], some uint8 [n_states]): views of an index."""
    stride = (int(n_words) + 3) & ~3
    cut = int(n_states) * stride * 4
    return index[:cut].view(torch.int32).view(int(n_states), stride), index[cut:cut + int(n_states)]


def dfa_step_device(tok: Tokenizer, ids: Optional[torch.Tensor], lengths: Optional[torch.Tensor], state: torch.Tensor, table: torch.Tensor,
                    index: torch.Tensor, *, end_ids, n_states: Optional[int] = None, keep_free: bool = False, mask: Optional[torch.Tensor] = None,
                    state_out: Optional[torch.Tensor] = None, live: Optional[torch.Tensor] = None, n_words: Optional[int] = None):
    """The regex guide, one step (spl_dfa_step_device), on torch's current stream; nothing synchronises.  state int64 [B]: the words as
    include/splintr_hip.h lays them out (dfa_state: the start states of sequences that begin); table: dfa_table(...); index:
    dfa_index_device(...) with the same n_words; ids [B] or [B, K] int32 / int64: what the sampler drew (a sequence's first lengths[b]
    entries count, all with lengths None); None: no ids, the masks of the state words as they are -- the first call after dfa_state.  An
    ordinary id whose bytes the automaton can walk moves the state; an END id (end_ids: 1 .. 8 ids, usually specials) in an accepting
    state ends the sequence (`done`); anything else breaks it (it runs free, `broken` set).  Returns (state_out int64 [B], mask int32
    [B, n_words], live uint8 [B]: 1 where the sequence is constrained after the call).  state_out may be state.  keep_free: rows of
    sequences that are not constrained after the call are not written -- pass the mask whose rows hold ones for them already.  n_states:
    default, the table's; n_words: default dfa_n_words(tok), or mask's."""
    if n_states is None:
        if not isinstance(table, torch.Tensor) or table.dim() != 1 or table.shape[0] % 513:
            raise ValueError("table must be a contiguous uint8 tensor of shape [n_states * 513] (dfa_table)")
        n_states = int(table.shape[0]) // 513
    if ids is None:
        if not isinstance(state, torch.Tensor) or state.dim() != 1:
            raise ValueError("state must be a contiguous int64 tensor of shape [batch]")
        ids = torch.empty((state.shape[0], 0), dtype=torch.int32, device=state.device)
    if mask is None and n_words is None:
        n_words = dfa_n_words(tok)
    check_dfa_args(ids, lengths, state, table, index, n_states, end_ids=end_ids, n_words=n_words, keep_free=keep_free, mask=mask, state_out=state_out)
    dev = ids.device
    B = int(ids.shape[0])
    K = int(ids.shape[1]) if ids.dim() == 2 else 1
    n_words = int(mask.shape[1]) if mask is not None else int(n_words)
    ends = _dfa_end_ids(end_ids, n_words)
    if mask is None:
        mask = torch.empty((B, n_words), dtype=torch.int32, device=dev)          # (every word of every row is written by the kernel)
    if state_out is None:
        state_out = torch.empty(B, dtype=torch.int64, device=dev)
    if live is None:
        live = torch.empty(max(B, 1), dtype=torch.uint8, device=dev)[:B]
    else:
        _vec("live", live, B, (torch.uint8,), "uint8")
    flags = (_ffi.SPL_DFA_KEEP_FREE if keep_free else 0) | (_ffi.SPL_DFA_I64 if ids.dtype == torch.int64 else 0)
    # (null state and mask pointers are refused by the library: an empty batch passes addresses of its own, which nothing dereferences)
    spare = torch.empty(8, dtype=torch.int64, device=dev).data_ptr() if B == 0 else 0
    si = _ffi.SplDfaIn(B, K, _ptr(ids), _ptr(lengths), _ptr(state) or spare, _ptr(table), _ptr(index), int(n_states))
    o = _ffi.SplDfaOpts(flags, n_words, ends)
    so = _ffi.SplDfaOut(_ptr(state_out) or spare + 16, _ptr(mask) or spare + 32, _ptr(live))
    rc = _ffi.lib().spl_dfa_step_device(tok.handle, ctypes.byref(si), ctypes.byref(o), ctypes.byref(so), torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        _raise_rc(rc, "spl_dfa_step_device")
    return state_out, mask, live


def dfa_jump_index_device(tok: Tokenizer, table: torch.Tensor, n_states: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The jump index of a DFA table (spl_dfa_jump_index_device): the forced byte run of every state, found on the GPU and encoded once by
    this tokenizer's own encoder, on torch's current stream.  BUILD-TIME work: the call may allocate and synchronises the stream once.
    Returns uint8 [n_states * 322]: int32 ids[n_states][64], uint8 n_ids[n_states], uint8 run_len[n_states], uint8 run[n_states][64]
    (dfa_jump_index_views gives the four views).  Build it again after add_special_tokens."""
    _dfa_check_table(table, n_states)
    if not table.is_cuda:
        raise ValueError("table must be on a GPU (dfa_table)")
    want = _ffi.SPL_DFA_JUMP_INDEX_BYTES(int(n_states))
    if out is None:
        out = torch.empty(want, dtype=torch.uint8, device=table.device)           # (every byte is written by the kernels)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.shape != (want,) or not out.is_contiguous() or out.device != table.device:
        raise ValueError(f"out must be a contiguous uint8 tensor of shape [{want}] on the device of the table")
    rc = _ffi.lib().spl_dfa_jump_index_device(tok.handle, _ptr(table), int(n_states), _ptr(out), torch.cuda.current_stream(table.device).cuda_stream)
    if rc != 0:
        _raise_rc(rc, "spl_dfa_jump_index_device")
    return out


def dfa_jump_index_views(index: torch.Tensor, n_states: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(ids int32 [n_states, 64], n_ids uint8 [n_states], run_len uint8 [n_states], run uint8 [n_states, 64]): views of a jump index (a
    tensor on the host or on the device whose storage is 4-byte aligned)."""
    S = int(n_states)
    if not isinstance(index, torch.Tensor) or index.dtype != torch.uint8 or index.shape != (_ffi.SPL_DFA_JUMP_INDEX_BYTES(S),) or not index.is_contiguous():
        raise ValueError(f"the jump index must be a contiguous uint8 tensor of shape [{_ffi.SPL_DFA_JUMP_INDEX_BYTES(S)}] (dfa_jump_index_device)")
    return index[:256 * S].view(torch.int32).view(S, 64), index[256 * S:257 * S], index[257 * S:258 * S], index[258 * S:].view(S, 64)


def check_dfa_jump_args(ids, lengths, state, table, index, jump_index, n_states, *, end_ids=None, n_words=None, keep_free: bool = False, mask=None,
                        state_out=None, forced_ids=None, forced_len=None, row_len_out=None) -> None:
    """ValueError for whatever dfa_jump_device would refuse -- check_dfa_args, and the jump index, the rows of emitted ids and their
    width -- before anything goes to the device."""
    check_dfa_args(ids, lengths, state, table, index, n_states, end_ids=end_ids, n_words=n_words, keep_free=keep_free, mask=mask, state_out=state_out)
    B = int(ids.shape[0])
    want = _ffi.SPL_DFA_JUMP_INDEX_BYTES(int(n_states))
    if not isinstance(jump_index, torch.Tensor) or jump_index.dtype != torch.uint8 or jump_index.shape != (want,) or not jump_index.is_contiguous():
        raise ValueError(f"jump_index must be a contiguous uint8 tensor of shape [{want}] (dfa_jump_index_device with the same n_states)")
    if jump_index.device != ids.device:
        raise ValueError("jump_index must be on the device of the ids")
    if forced_ids is not None:
        if not isinstance(forced_ids, torch.Tensor) or forced_ids.dtype != torch.int32 or forced_ids.dim() != 2 or forced_ids.shape[0] != B or \
                not forced_ids.is_contiguous() or forced_ids.device != ids.device:
            raise ValueError("forced_ids must be a contiguous int32 tensor of shape [batch, row_len_out] on the device of the ids")
        if row_len_out is not None and int(row_len_out) != int(forced_ids.shape[1]):
            raise ValueError("row_len_out must be the width of forced_ids")
        row_len_out = int(forced_ids.shape[1])
    if isinstance(row_len_out, bool) or not isinstance(row_len_out, (int, np.integer)) or not 1 <= int(row_len_out) <= _ffi.SPL_DFA_JUMP_MAX_IDS:
        raise ValueError(f"row_len_out (the width of forced_ids) must be an integer in 1 .. {_ffi.SPL_DFA_JUMP_MAX_IDS}, not {row_len_out!r}")
    if forced_len is not None:
        if _vec("forced_len", forced_len, B, (torch.int32,), "int32")[1].device != ids.device:
            raise ValueError("forced_len must be on the device of the ids")


def dfa_jump_device(tok: Tokenizer, ids: Optional[torch.Tensor], lengths: Optional[torch.Tensor], state: torch.Tensor, table: torch.Tensor,
                    index: torch.Tensor, jump_index: torch.Tensor, *, end_ids, n_states: Optional[int] = None, keep_free: bool = False,
                    mask: Optional[torch.Tensor] = None, state_out: Optional[torch.Tensor] = None, live: Optional[torch.Tensor] = None,
                    n_words: Optional[int] = None, forced_ids: Optional[torch.Tensor] = None, forced_len: Optional[torch.Tensor] = None,
                    row_len_out: Optional[int] = None):
    """The regex guide's step WITH jump-forward (spl_dfa_jump_device), on torch's current stream; nothing synchronises.  Everything
    dfa_step_device does, from the same arguments, and behind the sampler's ids the forced run of the state arrived at, as ids:
    jump_index is dfa_jump_index_device(...) of the same table.  Returns (state_out, mask, live, forced_ids int32 [B, row_len_out],
    forced_len int32 [B]): a sequence's first forced_len[b] entries of forced_ids[b] are ids the model need not be asked for -- the state
    and the mask are those BEHIND them; entries at and beyond forced_len[b] are not written.  row_len_out: 1 .. 64, default 16 (or the
    width of forced_ids); a run that does not fit is continued by the next call."""
    if n_states is None:
        if not isinstance(table, torch.Tensor) or table.dim() != 1 or table.shape[0] % 513:
            raise ValueError("table must be a contiguous uint8 tensor of shape [n_states * 513] (dfa_table)")
        n_states = int(table.shape[0]) // 513
    if ids is None:
        if not isinstance(state, torch.Tensor) or state.dim() != 1:
            raise ValueError("state must be a contiguous int64 tensor of shape [batch]")
        ids = torch.empty((state.shape[0], 0), dtype=torch.int32, device=state.device)
    if mask is None and n_words is None:
        n_words = dfa_n_words(tok)
    if forced_ids is None and row_len_out is None:
        row_len_out = 16
    check_dfa_jump_args(ids, lengths, state, table, index, jump_index, n_states, end_ids=end_ids, n_words=n_words, keep_free=keep_free, mask=mask,
                        state_out=state_out, forced_ids=forced_ids, forced_len=forced_len, row_len_out=row_len_out)
    dev = ids.device
    B = int(ids.shape[0])
    K = int(ids.shape[1]) if ids.dim() == 2 else 1
    n_words = int(mask.shape[1]) if mask is not None else int(n_words)
    ends = _dfa_end_ids(end_ids, n_words)
    if mask is None:
        mask = torch.empty((B, n_words), dtype=torch.int32, device=dev)          # (every word of every row is written by the kernel)
    if state_out is None:
        state_out = torch.empty(B, dtype=torch.int64, device=dev)
    if live is None:
        live = torch.empty(max(B, 1), dtype=torch.uint8, device=dev)[:B]
    else:
        _vec("live", live, B, (torch.uint8,), "uint8")
    if forced_ids is None:
        forced_ids = torch.zeros((B, int(row_len_out)), dtype=torch.int32, device=dev)   # (entries behind forced_len are not written: zeros)
    if forced_len is None:
        forced_len = torch.empty(max(B, 1), dtype=torch.int32, device=dev)[:B]
    flags = (_ffi.SPL_DFA_KEEP_FREE if keep_free else 0) | (_ffi.SPL_DFA_I64 if ids.dtype == torch.int64 else 0)
    # (null pointers are refused by the library: an empty batch passes addresses of its own, which nothing dereferences)
    spare = torch.empty(16, dtype=torch.int64, device=dev).data_ptr() if B == 0 else 0
    si = _ffi.SplDfaIn(B, K, _ptr(ids), _ptr(lengths), _ptr(state) or spare, _ptr(table), _ptr(index), int(n_states))
    o = _ffi.SplDfaOpts(flags, n_words, ends)
    so = _ffi.SplDfaOut(_ptr(state_out) or spare + 16, _ptr(mask) or spare + 32, _ptr(live))
    jo = _ffi.SplDfaJumpOut(int(forced_ids.shape[1]), _ptr(jump_index), _ptr(forced_ids) or spare + 48, _ptr(forced_len) or spare + 64)
    rc = _ffi.lib().spl_dfa_jump_device(tok.handle, ctypes.byref(si), ctypes.byref(o), ctypes.byref(so), ctypes.byref(jo),
                                        torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        _raise_rc(rc, "spl_dfa_jump_device")
    return state_out, mask, live, forced_ids, forced_len


class RegexGuide:
    """`tokenizer.regex_guide(batch_size, pattern)`: "the answer matches this regular expression" for a batch whose state lives on the
    GPU.  The pattern (or each of a list of patterns, stacked into one table) is compiled on the host by splintr_amd.dfa.compile_regex
    -- Python `re` semantics in bytes mode, fullmatch -- and its state x vocabulary index is built on the GPU once.  begin(select) writes
    the start states and the first masks; step(ids) follows the sampler; `mask` (int32 [B, n_words], the apply_token_bitmask layout)
    always holds the ids the next step may draw -- all ones for a sequence that is free, done or broken.  A sequence is done when an END
    id follows an accepting state.  UTF-8 validity of `.` and negated classes is not the guide's:
    DeviceStreamingDecoder.allowed_mask(guide.mask, and_into=True) ANDs it in.  Nothing here synchronises.

    jump=True adds JUMP-FORWARD: the constructor also builds the jump index (the forced byte run of every state, encoded once -- build-time
    work that synchronises once), and jump(ids) is step(ids) that also hands back, as ids, the run the automaton forces behind them:
    `forced_ids` int32 [B, jump_ids] and `forced_len` int32 [B] -- tokens no forward pass is needed for."""

    def __init__(self, tok: Tokenizer, batch_size: int, pattern_or_patterns, *, end_ids, n_words: Optional[int] = None, jump: bool = False,
                 jump_ids: int = 16):
        from . import dfa as _dfa
        if isinstance(batch_size, bool) or not isinstance(batch_size, (int, np.integer)) or not 0 <= int(batch_size) < (1 << 31):
            raise ValueError(f"batch_size must be an integer in 0 .. 2**31 - 1, not {batch_size!r}")
        self._tok, self.batch_size = tok, int(batch_size)
        self.n_words = dfa_n_words(tok) if n_words is None else int(n_words)
        _dfa_check_n_words(self.n_words)
        single = isinstance(pattern_or_patterns, (str, bytes, bytearray, _dfa.ByteDFA))
        pats = [pattern_or_patterns] if single else list(pattern_or_patterns)
        if not pats:
            raise ValueError("at least one pattern is needed")
        self.dfas = [p if isinstance(p, _dfa.ByteDFA) else _dfa.compile_regex(p) for p in pats]
        self.dfa, self.starts = _dfa.stack(self.dfas)
        self.n_states = self.dfa.n_states
        self.end_ids = _dfa_end_ids(end_ids, self.n_words)
        dev = torch.device("cuda", tok._device)
        dfa_reserve(tok)
        self.table = dfa_table(self.dfa, dev)
        self.index = dfa_index_device(tok, self.table, self.n_states, n_words=self.n_words)
        self.mask = torch.full((self.batch_size, self.n_words), -1, dtype=torch.int32, device=dev)
        self._state = torch.zeros(self.batch_size, dtype=torch.int64, device=dev)
        self.live = torch.zeros(self.batch_size, dtype=torch.uint8, device=dev)
        self.jump_index = self.forced_ids = self.forced_len = self._runs = None
        if jump:
            if isinstance(jump_ids, bool) or not isinstance(jump_ids, (int, np.integer)) or not 1 <= int(jump_ids) <= _ffi.SPL_DFA_JUMP_MAX_IDS:
                raise ValueError(f"jump_ids must be an integer in 1 .. {_ffi.SPL_DFA_JUMP_MAX_IDS}, not {jump_ids!r}")
            self.jump_index = dfa_jump_index_device(tok, self.table, self.n_states)
            self.forced_ids = torch.zeros((self.batch_size, int(jump_ids)), dtype=torch.int32, device=dev)
            self.forced_len = torch.zeros(self.batch_size, dtype=torch.int32, device=dev)
            _, _, run_len, run = dfa_jump_index_views(self.jump_index.cpu(), self.n_states)      # (the host copy forced_text answers from)
            self._runs = [bytes(run[q, :int(run_len[q])].tolist()) for q in range(self.n_states)]

    def _call(self, ids, lengths, keep_free):
        dfa_step_device(self._tok, ids, lengths, self._state, self.table, self.index, end_ids=self.end_ids, n_states=self.n_states,
                        keep_free=keep_free, mask=self.mask, state_out=self._state, live=self.live)
        return self.mask

    def begin(self, select=None, rows=None) -> torch.Tensor:
        """The start states of sequences that begin, and the first masks -> the mask.  select: None (every sequence: pattern 0), or per
        sequence the index of its pattern (None: the sequence runs free).  rows: the sequences that begin (indices or a bool mask; select
        then has one entry per such sequence); the others keep their state."""
        dev = self._state.device

        def words(sel, n):
            sel = [0] * n if sel is None else list(sel)
            if len(sel) != n:
                raise ValueError(f"select must have one entry per sequence that begins ({n}), not {len(sel)}")
            for b, p in enumerate(sel):
                if p is not None and (isinstance(p, bool) or not isinstance(p, (int, np.integer)) or not 0 <= int(p) < len(self.starts)):
                    raise ValueError(f"select {b} names pattern {p!r}: patterns are 0 .. {len(self.starts) - 1}")
            return torch.from_numpy(_dfa_state_host([None if p is None else self.starts[int(p)] for p in sel])).to(dev)

        if rows is None:
            self._state.copy_(words(select, self.batch_size), non_blocking=True)
        else:
            idx = torch.as_tensor(rows, device=dev)
            idx = idx.nonzero().flatten() if idx.dtype == torch.bool else idx.to(torch.int64).flatten()
            self._state[idx] = words(select, int(idx.numel()))
        return self._call(None, None, False)

    def step(self, ids: Optional[torch.Tensor], lengths: Optional[torch.Tensor] = None, *, keep_free: bool = False) -> torch.Tensor:
        """What the sampler drew, [B] or [B, K] (None: only the masks, after the caller wrote words into `state`) -> the mask.  keep_free:
        the rows of sequences that are not constrained are not written again -- right once a step WITHOUT it has run after the last
        sequence left its constraint (its row holds ones since then)."""
        return self._call(ids, lengths, keep_free)

    def jump(self, ids: Optional[torch.Tensor] = None, lengths: Optional[torch.Tensor] = None, *, keep_free: bool = False):
        """step(ids, lengths) with jump-forward (a guide made with jump=True) -> (forced_ids int32 [B, jump_ids], forced_len int32 [B]):
        behind what the sampler drew, the leading forced_len[b] entries of forced_ids[b] are the ids the automaton forces -- append them
        to the sequence without a forward pass; `mask`, `state` and `live` are those BEHIND them.  ids None right after begin() emits the
        start state's run.  A run longer than jump_ids ids (or 64 bytes) is continued by the next call: call jump(None) again while
        forced_len is not zero, or simply go on -- the mask allows nothing but the run.  The pair has the [B, K] + lengths form the
        streaming decoder takes:

            forced, n = guide.jump(drawn)                       # drawn: [B] from the sampler
            text = decoder.add_tokens(forced, lengths=n)        # DeviceStreamingDecoder: the run's text, no host round trip

        The ids are those of the run encoded alone: the seam with the text in front of it is not re-tokenised."""
        if self.jump_index is None:
            raise ValueError("this guide was made without jump=True")
        dfa_jump_device(self._tok, ids, lengths, self._state, self.table, self.index, self.jump_index, end_ids=self.end_ids, n_states=self.n_states,
                        keep_free=keep_free, mask=self.mask, state_out=self._state, live=self.live, forced_ids=self.forced_ids,
                        forced_len=self.forced_len)
        return self.forced_ids, self.forced_len

    def draft(self, ids: torch.Tensor, lengths: Optional[torch.Tensor] = None, parent: Optional[torch.Tensor] = None, *, states: bool = False,
              keep_free: bool = False) -> DraftResult:
        """A speculative sampler's draft, ids [B, K] with K <= 64 -- a chain (parent None) or a tree (parent int32 [K] or [B, K]: -1 or the
        index of an earlier node) -> DraftResult, in ONE launch (dfa_draft_device): mask [B, 1 + K, n_words] -- row 0 in front of the first
        draft id, row 1 + i behind node i, which is what apply(logits, mask=...) takes for the verifier's [B * (1 + K), V] logits --, ok
        [B, K], live [B, 1 + K] and, with states=True, the state behind every node.  The guide's own state, mask and live are untouched:

            d = guide.draft(drafted)                                   # drafted: [B, K] from the draft model
            guide.apply(logits.view(B * (1 + K), V), mask=d.mask)      # the verifier's logits, every position masked
            n = torch.minimum(d.accepted_len(), model_accepts)         # the leading ids both accept
            guide.accept(accepted_then_bonus, n + 1)                   # [B, K + 1]: the accepted ids, then the bonus id -- ONE step

        keep_free: the mask is made of ones and the rows of nodes that are not constrained are not written."""
        _guide_draft_ids(self, ids)
        mask = torch.full((self.batch_size, 1 + int(ids.shape[1]), self.n_words), -1, dtype=torch.int32, device=self._state.device) if keep_free else None
        return dfa_draft_device(self._tok, ids, lengths, self._state, self.table, self.index, end_ids=self.end_ids, parent=parent, n_states=self.n_states,
                                keep_free=keep_free, states=states, mask=mask, n_words=self.n_words)

    def accept(self, ids: Optional[torch.Tensor], lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The ordinary step under the name a speculative loop wants: the accepted draft ids and the bonus id in one call -> the mask."""
        return self._call(ids, lengths, False)

    def accept_node(self, draft: DraftResult, node) -> torch.Tensor:
        """The guide adopts the state behind node[b] of a draft made with states=True (-1: the root -- nothing was accepted) -> the mask.
        A gather of the draft's state, mask and live rows; no step is run."""
        return _guide_accept_node(self, draft, node)

    def forced_text(self, q: int) -> bytes:
        """The bytes state q (of the stacked table) forces: run(q) of include/splintr_hip.h, capped at 64 bytes and trimmed to a character
        boundary; b"" where the state leaves a choice or accepts.  From a host copy made at construction."""
        if self._runs is None:
            raise ValueError("this guide was made without jump=True")
        if isinstance(q, bool) or not isinstance(q, (int, np.integer)) or not 0 <= int(q) < self.n_states:
            raise ValueError(f"q must be a state in 0 .. {self.n_states - 1}, not {q!r}")
        return self._runs[int(q)]

    def reset(self, rows=None) -> None:
        """All sequences (rows None) or the given ones (indices or a bool mask) free, their mask rows ones."""
        if rows is None:
            self._state.zero_(); self.mask.fill_(-1); self.live.zero_()
            if self.forced_len is not None:
                self.forced_len.zero_()
        else:
            self._state[rows] = 0
            self.mask[rows] = -1
            self.live[rows] = 0
            if self.forced_len is not None:
                self.forced_len[rows] = 0

    def apply(self, logits: torch.Tensor, *, live_only: bool = False, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """logits [B, V] (float32, float16 or bfloat16) with -inf wherever the mask forbids the id, IN PLACE: one launch of
        mask_apply_device.  live_only: the rows of sequences that are not constrained (`live` 0) are skipped -- their mask rows hold ones,
        so the result is the same.  mask: a draft's mask [B, 1 + K, n_words] in place of the guide's own, for logits [B * (1 + K), V]."""
        return _guide_apply(self, logits, mask, live_only)

    @property
    def state(self) -> torch.Tensor:
        """int64 [B] on the device, as include/splintr_hip.h lays it out (the guide's own tensor: a word written here counts)"""
        return self._state

    @property
    def q(self) -> torch.Tensor:
        """int64 [B] on the device: the automaton's state of a constrained or done sequence (in the stacked table)"""
        return self._state & 0xFFFF

    @property
    def broken(self) -> torch.Tensor:
        return ((self._state >> 17) & 1).bool()

    @property
    def done(self) -> torch.Tensor:
        return ((self._state >> 18) & 1).bool()

    def __repr__(self) -> str:
        return f"RegexGuide(batch_size={self.batch_size}, patterns={len(self.dfas)}, n_states={self.n_states}, n_words={self.n_words})"


# ---------------------------------------------------------------------------------------------- nested languages: JSON mode (masks from a byte automaton with a stack)
def _nest_of(table):
    from . import nest as _nest
    if isinstance(table, _nest.NestTable):
        return table
    if hasattr(table, "trans") and not hasattr(table, "op"):
        return _nest.from_dfa(table)
    raise ValueError("the table must be a splintr_amd.nest.NestTable (json_table, from_dfa) or a splintr_amd.dfa.ByteDFA")


def nest_table(table, device=None) -> torch.Tensor:
    """The nest table of spl_nest_index_device / spl_nest_step_device on the device (default: the current GPU): uint8 [S * 769 + n_ret *
    32] -- uint16 trans[S][256], uint16 ret[n_ret][16], uint8 op[S][256], uint8 accept[S].  table: a splintr_amd.nest.NestTable, or a
    splintr_amd.dfa.ByteDFA (every op zero).  The tensor is the caller's."""
    return torch.from_numpy(_nest_of(table).table()).to(torch.device("cuda") if device is None else device)


def _nest_state_host(starts) -> np.ndarray:
    words = _dfa_state_host(starts)
    rows = np.zeros((len(words), _ffi.SPL_NEST_STATE_WORDS), dtype=np.int64)
    rows[:, 0] = words
    return rows


def nest_state(starts, device=None) -> torch.Tensor:
    """State rows int64 [len(starts), 5] for sequences that begin with an empty stack: per sequence a start state or None (a free row),
    built on the host -- nest_step_device with ids None then writes the first masks."""
    return torch.from_numpy(_nest_state_host(starts)).to(torch.device("cuda") if device is None else device)


def nest_reserve(tok: Tokenizer) -> None:
    """spl_nest_reserve_device: the decode tables and token healing's id -> rank on the device (shared with dfa_reserve); nest_step_device
    calls then neither allocate nor synchronise."""
    rc = _ffi.lib().spl_nest_reserve_device(tok.handle)
    if rc != 0:
        _raise_rc(rc, "spl_nest_reserve_device")


def _nest_check_table(table, n_states, n_ret):
    if isinstance(n_states, bool) or not isinstance(n_states, (int, np.integer)) or not 1 <= int(n_states) <= _ffi.SPL_NEST_MAX_STATES:
        raise ValueError(f"n_states must be an integer in 1 .. {_ffi.SPL_NEST_MAX_STATES}, not {n_states!r}")
    if isinstance(n_ret, bool) or not isinstance(n_ret, (int, np.integer)) or not 0 <= int(n_ret) <= _ffi.SPL_NEST_MAX_RET:
        raise ValueError(f"n_ret must be an integer in 0 .. {_ffi.SPL_NEST_MAX_RET}, not {n_ret!r}")
    want = _ffi.SPL_NEST_TABLE_BYTES(int(n_states), int(n_ret))
    if not isinstance(table, torch.Tensor) or table.dtype != torch.uint8 or table.shape != (want,) or not table.is_contiguous():
        raise ValueError(f"table must be a contiguous uint8 tensor of shape [{want}] (nest_table) for {int(n_states)} states and {int(n_ret)} ret rows")


def nest_index_device(tok: Tokenizer, table: torch.Tensor, n_states: int, n_ret: int, *, n_words: Optional[int] = None,
                      dep_cap: Optional[int] = None) -> Tuple[torch.Tensor, int]:
    """The index of a nest table (spl_nest_index_device), built on the GPU on torch's current stream -> (index uint8
    [SPL_NEST_INDEX_BYTES(n_states, n_words, n_dep)], n_dep): the stack-free rows, per state the ascending ids that touch the stack, and
    some[] -- nest_index_views gives the views.  BUILD-TIME work: the call may allocate and synchronises the stream.  dep_cap: a guess
    at the number of dependent entries (default 4096); where it is too small the build is repeated with the exact size, and an index
    built larger is cut to it.  n_words: default dfa_n_words(tok).  Build it again after add_special_tokens."""
    _nest_check_table(table, n_states, n_ret)
    _dfa_check_n_words(n_words)
    if not table.is_cuda:
        raise ValueError("table must be on a GPU (nest_table)")
    if dep_cap is not None and (isinstance(dep_cap, bool) or not isinstance(dep_cap, (int, np.integer)) or not 0 <= int(dep_cap) < (1 << 32)):
        raise ValueError(f"dep_cap must be an integer in 0 .. 2**32 - 1, not {dep_cap!r}")
    n_words = dfa_n_words(tok) if n_words is None else int(n_words)
    cap = 4096 if dep_cap is None else int(dep_cap)
    n_dep = ctypes.c_uint32(0)
    for _ in range(2):
        out = torch.empty(_ffi.SPL_NEST_INDEX_BYTES(int(n_states), n_words, cap), dtype=torch.uint8, device=table.device)
        rc = _ffi.lib().spl_nest_index_device(tok.handle, _ptr(table), int(n_states), int(n_ret), n_words, _ptr(out), cap, ctypes.byref(n_dep),
                                              torch.cuda.current_stream(table.device).cuda_stream)
        if rc != _ffi.SPL_ECAPACITY or n_dep.value <= cap:
            break
        cap = int(n_dep.value)                                                   # (the exact size)
    if rc != 0:
        _raise_rc(rc, "spl_nest_index_device")
    n = int(n_dep.value)
    if n < cap:                                                                  # some[] moves up behind the entries in use
        S, head = int(n_states), _ffi.SPL_NEST_INDEX_BYTES(int(n_states), n_words, 0) - int(n_states)
        out = torch.cat([out[:head + 4 * n], out[head + 4 * cap:head + 4 * cap + S]])
    return out, n


def nest_index_views(index: torch.Tensor, n_states: int, n_words: int, dep_cap: int):
    """(rows int32 [n_states, stride], dep_off int32 [n_states + 1], dep_ids int32 [dep_cap], some uint8 [n_states]): views of an index."""
    S, stride, cap = int(n_states), (int(n_words) + 3) & ~3, int(dep_cap)
    a = S * stride * 4
    b = a + 4 * (S + 1)
    c = b + 4 * cap
    return index[:a].view(torch.int32).view(S, stride), index[a:b].view(torch.int32), index[b:c].view(torch.int32), index[c:c + S]


def check_nest_args(ids, lengths, state, table, index, n_states, n_ret, dep_cap, *, end_ids=None, max_depth=64, n_words=None, keep_free: bool = False,
                    mask=None, state_out=None) -> None:
    """ValueError for a dtype, rank, shape, layout, size or device that nest_step_device would refuse -- before anything goes to the device."""
    if not isinstance(ids, torch.Tensor) or ids.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"the ids must be a torch tensor of dtype int32 or int64, not {getattr(ids, 'dtype', type(ids))}")
    if ids.dim() not in (1, 2):
        raise ValueError("the ids must have rank 1 ([batch]) or 2 ([batch, steps])")
    if not ids.is_contiguous():
        raise ValueError("the ids must be contiguous")
    B = int(ids.shape[0])
    if B >= (1 << 31) or (ids.dim() == 2 and ids.shape[1] >= (1 << 32)):
        raise ValueError("the sequences must be fewer than 2**31 and a row shorter than 2**32")
    if isinstance(max_depth, bool) or not isinstance(max_depth, (int, np.integer)) or not 1 <= int(max_depth) <= _ffi.SPL_NEST_MAX_DEPTH:
        raise ValueError(f"max_depth must be an integer in 1 .. {_ffi.SPL_NEST_MAX_DEPTH}, not {max_depth!r}")
    _dfa_check_n_words(n_words)
    _nest_check_table(table, n_states, n_ret)
    others = [("table", table)]
    if lengths is not None:
        others.append(_vec("lengths", lengths, B, (torch.int32,), "int32"))

    def rows(name, t):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.shape != (B, _ffi.SPL_NEST_STATE_WORDS) or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous int64 tensor of shape [batch, {_ffi.SPL_NEST_STATE_WORDS}]")
        return name, t

    others.append(rows("state", state))
    if state_out is not None:
        others.append(rows("state_out", state_out))
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.dtype != torch.int32 or mask.dim() != 2 or mask.shape[0] != B or not mask.is_contiguous() or \
                (n_words is not None and mask.shape[1] != int(n_words)):
            raise ValueError("mask must be a contiguous int32 tensor of shape [batch, n_words]")
        others.append(("mask", mask))
    elif keep_free:
        raise ValueError("keep_free needs the caller's mask (the rows of sequences that are not constrained filled with ones once)")
    width = int(mask.shape[1]) if mask is not None else int(n_words)
    want = _ffi.SPL_NEST_INDEX_BYTES(int(n_states), width, int(dep_cap))
    if not isinstance(index, torch.Tensor) or index.dtype != torch.uint8 or index.shape != (want,) or not index.is_contiguous():
        raise ValueError(f"index must be a contiguous uint8 tensor of shape [{want}] (nest_index_device with the same n_states and n_words, and its n_dep)")
    others.append(("index", index))
    _dfa_end_ids(end_ids, width)
    if not ids.is_cuda:
        raise ValueError("the ids must be on a GPU (the device-side nest guide takes no host tensor)")
    for name, t in others:
        if t.device != ids.device:
            raise ValueError(f"{name} must be on the device of the ids")


def nest_step_device(tok: Tokenizer, ids: Optional[torch.Tensor], lengths: Optional[torch.Tensor], state: torch.Tensor, table: torch.Tensor,
                     index: torch.Tensor, *, n_states: int, n_ret: int, dep_cap: int, end_ids, max_depth: int = 64, keep_free: bool = False,
                     mask: Optional[torch.Tensor] = None, state_out: Optional[torch.Tensor] = None, live: Optional[torch.Tensor] = None,
                     n_words: Optional[int] = None):
    """The nest guide, one step (spl_nest_step_device), on torch's current stream; nothing synchronises.  state int64 [B, 5]: the rows as
    include/splintr_hip.h lays them out (nest_state: sequences that begin); table: nest_table(...); index, dep_cap: what
    nest_index_device returned; ids [B] or [B, K] int32 / int64: what the sampler drew (None: no ids, the masks of the rows as they are).
    An ordinary id whose bytes the automaton can walk from the sequence's state AND STACK moves both; an END id in an accepting state
    with an empty stack ends the sequence; anything else breaks it.  Returns (state_out int64 [B, 5], mask int32 [B, n_words], live uint8
    [B]).  state_out may be state.  max_depth: the deepest stack, 1 .. 64 -- an opener beyond it is not allowed."""
    if ids is None:
        if not isinstance(state, torch.Tensor) or state.dim() != 2:
            raise ValueError(f"state must be a contiguous int64 tensor of shape [batch, {_ffi.SPL_NEST_STATE_WORDS}]")
        ids = torch.empty((state.shape[0], 0), dtype=torch.int32, device=state.device)
    if mask is None and n_words is None:
        n_words = dfa_n_words(tok)
    check_nest_args(ids, lengths, state, table, index, n_states, n_ret, dep_cap, end_ids=end_ids, max_depth=max_depth, n_words=n_words,
                    keep_free=keep_free, mask=mask, state_out=state_out)
    dev = ids.device
    B = int(ids.shape[0])
    K = int(ids.shape[1]) if ids.dim() == 2 else 1
    n_words = int(mask.shape[1]) if mask is not None else int(n_words)
    ends = _dfa_end_ids(end_ids, n_words)
    if mask is None:
        mask = torch.empty((B, n_words), dtype=torch.int32, device=dev)          # (every word of every row is written by the kernel)
    if state_out is None:
        state_out = torch.empty((B, _ffi.SPL_NEST_STATE_WORDS), dtype=torch.int64, device=dev)
    if live is None:
        live = torch.empty(max(B, 1), dtype=torch.uint8, device=dev)[:B]
    else:
        _vec("live", live, B, (torch.uint8,), "uint8")
    flags = (_ffi.SPL_NEST_KEEP_FREE if keep_free else 0) | (_ffi.SPL_NEST_I64 if ids.dtype == torch.int64 else 0)
    # (null state and mask pointers are refused by the library: an empty batch passes addresses of its own, which nothing dereferences)
    spare = torch.empty(8, dtype=torch.int64, device=dev).data_ptr() if B == 0 else 0
    si = _ffi.SplNestIn(B, K, _ptr(ids), _ptr(lengths), _ptr(state) or spare, _ptr(table), _ptr(index), int(n_states), int(n_ret), int(dep_cap),
                        int(index.numel()))
    o = _ffi.SplNestOpts(flags, n_words, ends, int(max_depth))
    so = _ffi.SplNestOut(_ptr(state_out) or spare + 16, _ptr(mask) or spare + 32, _ptr(live))
    rc = _ffi.lib().spl_nest_step_device(tok.handle, ctypes.byref(si), ctypes.byref(o), ctypes.byref(so), torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        _raise_rc(rc, "spl_nest_step_device")
    return state_out, mask, live


class NestGuide:
    """`tokenizer.nest_guide(batch_size, table)` / `tokenizer.json_guide(batch_size)`: "the answer is a word of this nested language" --
    JSON mode -- for a batch whose state AND STACK live on the GPU.  The table's index is built on the GPU once (build-time work that
    synchronises); begin() writes the start state and the first masks; step(ids) follows the sampler; `mask` (int32 [B, n_words], the
    apply_token_bitmask layout) always holds the ids the next step may draw -- all ones for a sequence that is free, done or broken.  A
    sequence is done when an END id follows an accepting state with an empty stack.  After the constructor nothing synchronises."""

    def __init__(self, tok: Tokenizer, batch_size: int, table, *, end_ids, max_depth: int = 64, n_words: Optional[int] = None):
        if isinstance(batch_size, bool) or not isinstance(batch_size, (int, np.integer)) or not 0 <= int(batch_size) < (1 << 31):
            raise ValueError(f"batch_size must be an integer in 0 .. 2**31 - 1, not {batch_size!r}")
        if isinstance(max_depth, bool) or not isinstance(max_depth, (int, np.integer)) or not 1 <= int(max_depth) <= _ffi.SPL_NEST_MAX_DEPTH:
            raise ValueError(f"max_depth must be an integer in 1 .. {_ffi.SPL_NEST_MAX_DEPTH}, not {max_depth!r}")
        self._tok, self.batch_size, self.max_depth = tok, int(batch_size), int(max_depth)
        self.n_words = dfa_n_words(tok) if n_words is None else int(n_words)
        _dfa_check_n_words(self.n_words)
        self.nest = _nest_of(table)
        self.n_states, self.n_ret, self.start = self.nest.n_states, self.nest.n_ret, self.nest.start
        self.end_ids = _dfa_end_ids(end_ids, self.n_words)
        dev = torch.device("cuda", tok._device)
        nest_reserve(tok)
        self.table = nest_table(self.nest, dev)
        self.index, self.n_dep = nest_index_device(tok, self.table, self.n_states, self.n_ret, n_words=self.n_words)
        self.mask = torch.full((self.batch_size, self.n_words), -1, dtype=torch.int32, device=dev)
        self._state = torch.zeros((self.batch_size, _ffi.SPL_NEST_STATE_WORDS), dtype=torch.int64, device=dev)
        self.live = torch.zeros(self.batch_size, dtype=torch.uint8, device=dev)

    def _call(self, ids, lengths, keep_free):
        nest_step_device(self._tok, ids, lengths, self._state, self.table, self.index, n_states=self.n_states, n_ret=self.n_ret, dep_cap=self.n_dep,
                         end_ids=self.end_ids, max_depth=self.max_depth, keep_free=keep_free, mask=self.mask, state_out=self._state, live=self.live)
        return self.mask

    def begin(self, rows=None) -> torch.Tensor:
        """The start state and an empty stack for every sequence (rows None) or the given ones (indices or a bool mask; the others keep
        their state), and the first masks -> the mask."""
        first = torch.zeros(_ffi.SPL_NEST_STATE_WORDS, dtype=torch.int64, device=self._state.device)
        first[0] = self.start | 1 << 16
        if rows is None:
            self._state.copy_(first.expand_as(self._state))
        else:
            self._state[rows] = first
        return self._call(None, None, False)

    def step(self, ids: Optional[torch.Tensor], lengths: Optional[torch.Tensor] = None, *, keep_free: bool = False) -> torch.Tensor:
        """What the sampler drew, [B] or [B, K] (None: only the masks, after the caller wrote rows into `state`) -> the mask.  keep_free:
        the rows of sequences that are not constrained are not written again -- right once a step WITHOUT it has run after the last
        sequence left its constraint (its row holds ones since then)."""
        return self._call(ids, lengths, keep_free)

    def reset(self, rows=None) -> None:
        """All sequences (rows None) or the given ones (indices or a bool mask) free, their mask rows ones."""
        if rows is None:
            self._state.zero_(); self.mask.fill_(-1); self.live.zero_()
        else:
            self._state[rows] = 0
            self.mask[rows] = -1
            self.live[rows] = 0

    def draft(self, ids: torch.Tensor, lengths: Optional[torch.Tensor] = None, parent: Optional[torch.Tensor] = None, *, states: bool = False,
              keep_free: bool = False) -> DraftResult:
        """RegexGuide.draft's, over configurations (nest_draft_device, ONE launch): the masks in front of and behind every node of a
        draft chain or tree, ok per node, live and -- with states=True -- the state and stack behind every node.  The guide's own state
        is untouched."""
        _guide_draft_ids(self, ids)
        mask = torch.full((self.batch_size, 1 + int(ids.shape[1]), self.n_words), -1, dtype=torch.int32, device=self._state.device) if keep_free else None
        return nest_draft_device(self._tok, ids, lengths, self._state, self.table, self.index, n_states=self.n_states, n_ret=self.n_ret, dep_cap=self.n_dep,
                                 end_ids=self.end_ids, max_depth=self.max_depth, parent=parent, keep_free=keep_free, states=states, mask=mask,
                                 n_words=self.n_words)

    def accept(self, ids: Optional[torch.Tensor], lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The ordinary step under the name a speculative loop wants: the accepted draft ids and the bonus id in one call -> the mask."""
        return self._call(ids, lengths, False)

    def accept_node(self, draft: DraftResult, node) -> torch.Tensor:
        """The guide adopts the state and stack behind node[b] of a draft made with states=True (-1: the root) -> the mask.  A gather of
        the draft's state, mask and live rows; no step is run."""
        return _guide_accept_node(self, draft, node)

    def apply(self, logits: torch.Tensor, *, live_only: bool = False, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """logits [B, V] (float32, float16 or bfloat16) with -inf wherever the mask forbids the id, IN PLACE: one launch of
        mask_apply_device.  live_only: the rows of sequences that are not constrained (`live` 0) are skipped.  mask: a draft's mask
        [B, 1 + K, n_words] in place of the guide's own, for logits [B * (1 + K), V]."""
        return _guide_apply(self, logits, mask, live_only)

    @property
    def state(self) -> torch.Tensor:
        """int64 [B, 5] on the device, as include/splintr_hip.h lays it out (the guide's own tensor: a row written here counts)"""
        return self._state

    @property
    def q(self) -> torch.Tensor:
        """int64 [B] on the device: the automaton's state of a constrained or done sequence"""
        return self._state[:, 0] & 0xFFFF

    @property
    def depth(self) -> torch.Tensor:
        """int64 [B] on the device: the open brackets of a constrained sequence"""
        return (self._state[:, 0] >> 24) & 0x7F

    @property
    def broken(self) -> torch.Tensor:
        return ((self._state[:, 0] >> 17) & 1).bool()

    @property
    def done(self) -> torch.Tensor:
        return ((self._state[:, 0] >> 18) & 1).bool()

    def stacks(self):
        """The stacks as tuples of symbols, the bottom first: a host copy (it synchronises)."""
        rows = self._state.cpu().numpy().view(np.uint64)
        return [tuple(int(r[1 + i // 16] >> np.uint64(4 * (i % 16))) & 15 for i in range(int(r[0] >> np.uint64(24)) & 0x7F)) for r in rows]

    def __repr__(self) -> str:
        return f"NestGuide(batch_size={self.batch_size}, n_states={self.n_states}, n_dep={self.n_dep}, max_depth={self.max_depth}, n_words={self.n_words})"


# ---------------------------------------------------------------------------------------------- draft verification: the guides behind a speculative sampler
class DraftResult:
    """What a draft call wrote: mask int32 [B, 1 + K, n_words] (row 0 in front of the first draft id, row 1 + i behind node i), ok uint8
    [B, K] (1: every id of the node's path is acceptable), live uint8 [B, 1 + K], state int64 [B, 1 + K] (regex) / [B, 1 + K, 5] (nest),
    or None where the states were not asked for."""

    def __init__(self, mask, ok, live, state, tree: bool):
        self.mask, self.ok, self.live, self.state, self.tree = mask, ok, live, state, bool(tree)

    def accepted_len(self) -> torch.Tensor:
        """int64 [B]: the leading draft ids of a CHAIN the guide accepts (ok is monotone along a chain, so this is its sum)."""
        if self.tree:
            raise ValueError("accepted_len is a chain's: a tree has no leading ids (read ok per node)")
        return self.ok.sum(1)

    def __repr__(self) -> str:
        return f"DraftResult(mask={tuple(self.mask.shape)}, states={self.state is not None}, tree={self.tree})"


def check_draft_args(ids, parent, *, keep_free: bool = False, mask=None, n_words=None, state_words: int = 1) -> None:
    """ValueError for what a draft call refuses beyond the step's own checks (check_dfa_args / check_nest_args run on the same ids): the
    ids must be [batch, nodes] with at most 64 nodes, the parents int32 [nodes] or [batch, nodes] on the device of the ids, the caller's
    mask [batch, 1 + nodes, n_words]."""
    if not isinstance(ids, torch.Tensor) or ids.dim() != 2:
        raise ValueError("the draft ids must have rank 2 ([batch, nodes])")
    B, K = int(ids.shape[0]), int(ids.shape[1])
    if K > _ffi.SPL_DRAFT_MAX_NODES:
        raise ValueError(f"a draft has at most {_ffi.SPL_DRAFT_MAX_NODES} nodes, not {K}")
    if (1 + K) * B >= (1 << 31):
        raise ValueError("(1 + nodes) * batch must be below 2**31")
    if parent is not None:
        if not isinstance(parent, torch.Tensor) or parent.dtype != torch.int32 or not parent.is_contiguous() or tuple(parent.shape) not in ((K,), (B, K)):
            raise ValueError("parent must be a contiguous int32 tensor of shape [nodes] (one tree for all sequences) or [batch, nodes]")
        if parent.device != ids.device:
            raise ValueError("parent must be on the device of the ids")
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.dtype != torch.int32 or mask.dim() != 3 or mask.shape[0] != B or mask.shape[1] != 1 + K or \
                not mask.is_contiguous() or (n_words is not None and mask.shape[2] != int(n_words)):
            raise ValueError("mask must be a contiguous int32 tensor of shape [batch, 1 + nodes, n_words]")
        if mask.device != ids.device:
            raise ValueError("mask must be on the device of the ids")
    elif keep_free:
        raise ValueError("keep_free needs the caller's mask (the rows of nodes that are not constrained filled with ones once)")


def _draft_out(ids, parent, keep_free, mask, n_words, states, state_shape):
    """the outputs of a draft call and its spl_draft_out (the tensors are returned too: they must outlive the call's arguments)"""
    dev, B, K = ids.device, int(ids.shape[0]), int(ids.shape[1])
    if mask is None:
        mask = torch.empty((B, 1 + K, n_words), dtype=torch.int32, device=dev)     # (every word of every row is written by the kernel)
    ok = torch.empty((B, K), dtype=torch.uint8, device=dev)
    live = torch.empty((B, 1 + K), dtype=torch.uint8, device=dev)
    state = torch.empty((B, 1 + K) + state_shape, dtype=torch.int64, device=dev) if states else None
    per_seq = parent is not None and parent.dim() == 2
    # (null mask and ok pointers are refused by the library: an empty batch or an empty draft passes addresses of its own, which nothing dereferences)
    spare = torch.empty(8, dtype=torch.int64, device=dev).data_ptr() if (B == 0 or K == 0) else 0
    d = _ffi.SplDraftOut(_ffi.SPL_DRAFT_PARENT_PER_SEQ if per_seq and parent.numel() else 0, _ptr(parent), _ptr(mask) or spare, _ptr(ok) or spare + 16,
                         _ptr(live), _ptr(state))
    return d, DraftResult(mask, ok, live, state, parent is not None)


def dfa_draft_device(tok: Tokenizer, ids: torch.Tensor, lengths: Optional[torch.Tensor], state: torch.Tensor, table: torch.Tensor, index: torch.Tensor, *,
                     end_ids, parent: Optional[torch.Tensor] = None, n_states: Optional[int] = None, keep_free: bool = False, states: bool = False,
                     mask: Optional[torch.Tensor] = None, n_words: Optional[int] = None) -> DraftResult:
    """The regex guide over a DRAFT (spl_dfa_draft_device), ONE launch on torch's current stream; nothing synchronises and `state` is only
    read.  ids [B, K] int32 / int64, K <= 64: the draft's nodes (a sequence's first lengths[b] count, the others are absent); parent None:
    a chain; int32 [K] or [B, K]: per node -1 (it hangs below the sequence's state) or the index of an earlier node.  Returns a
    DraftResult: mask row 0 is the mask in front of the first draft id, row 1 + i the mask behind node i; ok[b, i] is 1 iff every id on
    the way to node i is one the guide accepts; live and -- with states=True -- state hold what dfa_step_device would have written had it
    been given the node's path.  keep_free: the rows of nodes that are not constrained are not written -- pass the mask whose rows hold
    ones already."""
    if n_states is None:
        if not isinstance(table, torch.Tensor) or table.dim() != 1 or table.shape[0] % 513:
            raise ValueError("table must be a contiguous uint8 tensor of shape [n_states * 513] (dfa_table)")
        n_states = int(table.shape[0]) // 513
    if mask is None and n_words is None:
        n_words = dfa_n_words(tok)
    check_draft_args(ids, parent, keep_free=keep_free, mask=mask, n_words=n_words)
    n_words = int(mask.shape[2]) if mask is not None else int(n_words)
    check_dfa_args(ids, lengths, state, table, index, n_states, end_ids=end_ids, n_words=n_words)
    B, K = int(ids.shape[0]), int(ids.shape[1])
    ends = _dfa_end_ids(end_ids, n_words)
    d, res = _draft_out(ids, parent, keep_free, mask, n_words, states, ())
    flags = (_ffi.SPL_DFA_KEEP_FREE if keep_free else 0) | (_ffi.SPL_DFA_I64 if ids.dtype == torch.int64 else 0)
    spare = torch.empty(8, dtype=torch.int64, device=ids.device).data_ptr() if B == 0 else 0
    si = _ffi.SplDfaIn(B, K, _ptr(ids), _ptr(lengths), _ptr(state) or spare, _ptr(table), _ptr(index), int(n_states))
    o = _ffi.SplDfaOpts(flags, n_words, ends)
    rc = _ffi.lib().spl_dfa_draft_device(tok.handle, ctypes.byref(si), ctypes.byref(o), ctypes.byref(d), torch.cuda.current_stream(ids.device).cuda_stream)
    if rc != 0:
        _raise_rc(rc, "spl_dfa_draft_device")
    return res


def nest_draft_device(tok: Tokenizer, ids: torch.Tensor, lengths: Optional[torch.Tensor], state: torch.Tensor, table: torch.Tensor, index: torch.Tensor, *,
                      n_states: int, n_ret: int, dep_cap: int, end_ids, max_depth: int = 64, parent: Optional[torch.Tensor] = None, keep_free: bool = False,
                      states: bool = False, mask: Optional[torch.Tensor] = None, n_words: Optional[int] = None) -> DraftResult:
    """The nest guide over a DRAFT (spl_nest_draft_device): dfa_draft_device's, over configurations -- state int64 [B, 5] is only read, a
    DraftResult's state is int64 [B, 1 + K, 5]."""
    if mask is None and n_words is None:
        n_words = dfa_n_words(tok)
    check_draft_args(ids, parent, keep_free=keep_free, mask=mask, n_words=n_words)
    n_words = int(mask.shape[2]) if mask is not None else int(n_words)
    check_nest_args(ids, lengths, state, table, index, n_states, n_ret, dep_cap, end_ids=end_ids, max_depth=max_depth, n_words=n_words)
    B, K = int(ids.shape[0]), int(ids.shape[1])
    ends = _dfa_end_ids(end_ids, n_words)
    d, res = _draft_out(ids, parent, keep_free, mask, n_words, states, (_ffi.SPL_NEST_STATE_WORDS,))
    flags = (_ffi.SPL_NEST_KEEP_FREE if keep_free else 0) | (_ffi.SPL_NEST_I64 if ids.dtype == torch.int64 else 0)
    spare = torch.empty(8, dtype=torch.int64, device=ids.device).data_ptr() if B == 0 else 0
    si = _ffi.SplNestIn(B, K, _ptr(ids), _ptr(lengths), _ptr(state) or spare, _ptr(table), _ptr(index), int(n_states), int(n_ret), int(dep_cap),
                        int(index.numel()))
    o = _ffi.SplNestOpts(flags, n_words, ends, int(max_depth))
    rc = _ffi.lib().spl_nest_draft_device(tok.handle, ctypes.byref(si), ctypes.byref(o), ctypes.byref(d), torch.cuda.current_stream(ids.device).cuda_stream)
    if rc != 0:
        _raise_rc(rc, "spl_nest_draft_device")
    return res


def _guide_draft_ids(guide, ids):
    if not isinstance(ids, torch.Tensor) or ids.dim() != 2 or ids.shape[0] != guide.batch_size:
        raise ValueError("the draft ids must have shape [batch, nodes]")
    return ids


def _guide_accept_node(guide, draft: DraftResult, node) -> torch.Tensor:
    """the state, mask and live rows of node[b] (-1: the root) of a draft become the guide's: three gathers, no kernel of the library"""
    if not isinstance(draft, DraftResult):
        raise ValueError("draft must be what draft() returned")
    if draft.state is None:
        raise ValueError("accept_node needs the states behind the nodes: call draft(..., states=True)")
    B, rows = guide.batch_size, int(draft.mask.shape[1])
    if draft.mask.shape[0] != B or draft.mask.shape[2] != guide.n_words:
        raise ValueError("the draft is not this guide's")
    on_host = not (isinstance(node, torch.Tensor) and node.is_cuda)
    node = torch.as_tensor(node)
    if node.dtype not in (torch.int32, torch.int64) or node.shape != (B,):
        raise ValueError("node must hold one integer per sequence: -1 (the root) or a node of the draft")
    if on_host and B and (int(node.min()) < -1 or int(node.max()) > rows - 2):
        raise ValueError(f"node must be in -1 .. {rows - 2}")
    # (a tensor on the device is not read back: a value outside -1 .. nodes - 1 is clamped to that range, nothing synchronises)
    at = (node.to(guide._state.device, torch.int64) + 1).clamp_(0, rows - 1)
    b = torch.arange(B, device=at.device)
    guide._state.copy_(draft.state[b, at])
    guide.mask.copy_(draft.mask[b, at])
    guide.live.copy_(draft.live[b, at])
    return guide.mask


def _guide_apply(guide, logits, mask, live_only):
    """logits [R, V] against the guide's own mask (R = batch) or against the rows of a draft's mask ([B, 1 + K, n_words] or [R, n_words])"""
    if mask is None:
        if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.shape[0] != guide.batch_size:
            raise ValueError("logits must have shape [batch, vocabulary]")
        return mask_apply_device(guide._tok, logits, guide.mask, live=guide.live if live_only else None)
    if live_only:
        raise ValueError("live_only goes with the guide's own mask")
    if not isinstance(mask, torch.Tensor) or mask.dim() not in (2, 3) or mask.shape[-1] != guide.n_words or not mask.is_contiguous():
        raise ValueError("mask must be a contiguous tensor of shape [batch, 1 + nodes, n_words] (a draft's) or [rows, n_words]")
    rows = mask.view(-1, guide.n_words)
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.shape[0] != rows.shape[0]:
        raise ValueError("logits must have shape [rows of the mask, vocabulary]")
    return mask_apply_device(guide._tok, logits, rows)


class Comm:
    """One rank of the library's own RCCL communicator (include/splintr_hip.h: spl_comm_*).  The 128-byte id is
    made by rank 0 and handed to the others by whatever the caller has; `from_torch_group` uses an existing
    torch.distributed group (any backend: it only carries 128 bytes) for that."""

    def __init__(self, unique_id: bytes, rank: int, world: int, device: int):
        L = _ffi.lib()
        self._h = L.spl_comm_create(unique_id, rank, world, device)
        if not self._h:
            raise RuntimeError(f"spl_comm_create failed: {_ffi.last_error()}")
        self.rank, self.world, self.device = rank, world, device

    @staticmethod
    def unique_id() -> bytes:
        buf = ctypes.create_string_buffer(128)
        if _ffi.lib().spl_comm_unique_id(buf) != 0:
            raise RuntimeError(f"spl_comm_unique_id failed: {_ffi.last_error()}")
        return buf.raw

    @classmethod
    def from_torch_group(cls, device: torch.device, group=None) -> "Comm":
        import torch.distributed as dist
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        box = [cls.unique_id() if rank == 0 else None]
        if world > 1:
            dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        return cls(box[0], rank, world, device.index if device.index is not None else torch.cuda.current_device())

    @property
    def handle(self) -> int:
        return self._h

    def allgatherv_csr(self, ids: torch.Tensor, out_off: torch.Tensor, n_docs: int, all_ids: torch.Tensor,
                       all_off: torch.Tensor) -> Tuple[int, int]:
        """spl_allgatherv_csr on torch's current stream: exactly T_r ids and N_r offsets per rank, straight to
        their place of the global CSR.  Returns (total tokens, total documents); one host synchronisation."""
        nt, nd = ctypes.c_uint64(), ctypes.c_uint64()
        stream = torch.cuda.current_stream(ids.device).cuda_stream
        rc = _ffi.lib().spl_allgatherv_csr(self._h, ids.data_ptr(), out_off.data_ptr(), n_docs, all_ids.data_ptr(),
                                           all_ids.numel(), all_off.data_ptr(), all_off.numel(), ctypes.byref(nt),
                                           ctypes.byref(nd), stream)
        if rc != 0:
            raise RuntimeError(f"spl_allgatherv_csr failed ({rc}): {_ffi.last_error()}")
        return int(nt.value), int(nd.value)

    def ranks(self) -> int:
        """spl_comm_world: the number of ranks of the RCCL communicator the LIBRARY holds (what a scaling run checks
        against torch's world size)."""
        return int(_ffi.lib().spl_comm_world(self._h))

    def close(self) -> None:
        if getattr(self, "_h", None):
            _ffi.lib().spl_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _slab_words(max_tokens: int, max_docs: int, pack24: bool) -> int:
    """words of one slab: header, offsets, then the ids -- u32 each, or three bytes each (+ one word of slack for the unpacker's reads)"""
    return ((3 * max_tokens + 3) // 4 + 1 if pack24 else max_tokens) + max_docs + 4


_EXCH_STREAMS = {}


def exchange_stream(device: torch.device) -> "torch.cuda.Stream":
    """THE exchange stream of a device: one per process and GPU, shared by every GatherV / WaveGather on it.
    HIP maps streams onto a handful of hardware queues by what else the process has created: the n-th stream may land on the queue
    (or the command-processor pipe) the encoder's stream uses, and then the exchange runs BEHIND the encodes instead of beside them
    (measured: the fourth WaveGather of a process lost the whole overlap, 5.47 -> 6.05 ms per step).  The stream is therefore picked
    by measurement beside the stream that is current when it is first asked for (spl_pick_stream)."""
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    st = _EXCH_STREAMS.get(key)
    if st is None:
        st = _EXCH_STREAMS[key] = pick_stream(device, [torch.cuda.current_stream(device)])
    return st


def pick_stream(device: torch.device, beside) -> "torch.cuda.Stream":
    """A new stream that really runs beside the streams in `beside` (spl_pick_stream: measured, not assumed)."""
    import ctypes
    idx = device.index if device.index is not None else torch.cuda.current_device()
    arr = (ctypes.c_void_p * max(1, len(beside)))(*[ctypes.c_void_p(int(s.cuda_stream)) for s in beside])
    out, left = ctypes.c_void_p(), ctypes.c_double()
    if _ffi.lib().spl_pick_stream(idx, arr, len(beside), ctypes.byref(out), ctypes.byref(left)) != 0:
        raise RuntimeError(_ffi.last_error())
    st = torch.cuda.ExternalStream(out.value, device=device)
    st.conflict_us = left.value
    _PICKS.append({"beside": len(beside), "conflict_us": round(float(left.value), 1), "least_bad": bool(left.value >= PICK_CONFLICT_US)})
    return st


# Every stream this process picked by measurement, in order: what the candidate that was kept still lost to its neighbours (microseconds
# for four empty kernels beside a spinning stream, minus the same alone).  spl_pick_stream keeps the first candidate without a conflict and
# otherwise the LEAST BAD one -- silently, up to round 5; a scaling run records the picks and flags a leg that ran on a least-bad one.
PICK_CONFLICT_US = 15.0
_PICKS = []


def stream_picks():
    return list(_PICKS)


_ENC_STREAMS = {}


def encode_streams(device: torch.device, pair: int = 0):
    """Two streams per process and GPU on which WaveGather encodes consecutive waves in alternation -- pair `pair` of three pairs created
    once.  HIP multiplexes a process's streams onto a few hardware queues, and hardware queues onto four pipes of the command processor:
    two busy streams that end up on one pipe take turns instead of running side by side (kernel trace: every small kernel of such a stream
    takes 40 - 55 us instead of 4 - 13, the tile kernels 215 us instead of 130).  Which streams share is decided by what else the process has
    created; nothing in the HIP API tells.  The streams are therefore PICKED by measurement (spl_pick_stream) beside the exchange stream and
    each other; a caller that can afford a calibration still tries the pairs and keeps the fastest (bench.py)."""
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    st = _ENC_STREAMS.setdefault(key, {})
    p = pair % 3
    if p not in st:
        ex = exchange_stream(device)
        a = pick_stream(device, [ex])
        st[p] = (a, pick_stream(device, [ex, a]))
    return st[p]


def _set_pack24(tok: Optional[Tokenizer], on: bool, owner=None) -> None:
    """The slab format is the HANDLE's (spl_set_option "slab_pack24"), read by the encoder at every launch: a gatherer (re)asserts ITS format
    in front of each of its encodes and packs (one C call that stores an int), so that gatherers of both formats can live on one Tokenizer
    (one thread) without one silently changing the wire format of the other."""
    if tok is None:                              # the bucket logic driven without an encoder (CPU tests): slabs come from the caller
        return
    if _ffi.lib().spl_set_option(tok.handle, b"slab_pack24", 1 if on else 0) != 0:
        raise RuntimeError(_ffi.last_error())


class GatherV:
    """Pipelined, bucketed ragged all-gather of per-rank CSR results.

    Every batch is packed into a slab right after its encode (HIP kernel, same stream).  `depth`
    consecutive slabs form one bucket; a full bucket is handed to an exchange stream of its own:
    ONE all-gather of world x depth equal slabs (RCCL over xGMI: spl_allgather_slabs on the library's own
    communicator when `comm` is given, torch.distributed's all_gather_into_tensor otherwise) and ONE unpack launch
    that rebuilds the global CSR of each of the bucket's batches on every rank.  Two bucket SETS
    alternate -- each with its own send, receive and result buffers -- so the exchange of one bucket
    overlaps the encodes of the next and no cross-stream wait sits between two encodes.  Fewer,
    larger collectives on purpose: xGMI rings are per-link bound and a collective costs tens of
    microseconds of launch work, as much as encoding a whole 1 MB batch.

    Results: `on_bucket(results)` -- if set -- is called for every exchanged bucket with a list of
    (ids, off) views, one per batch in submission order (ids int32, the first off[-1] entries valid;
    off int64[world * max_docs + 1], entries past the global document count unspecified).  It runs
    with the exchange stream current: whatever it enqueues is ordered behind the unpack, and the
    set's buffers are reused only after that work.  `finish()` flushes a partial bucket, drains,
    and returns the views of the LAST submitted batch.  No host synchronisation per batch.
    """

    def __init__(self, tok: Tokenizer, device: torch.device, max_docs: int, max_tokens: int, group=None, depth: int = 8,
                 comm: "Comm" = None, collective: str = "allgather", pack24: bool = False):
        import torch.distributed as dist
        self.tok, self.dev, self.group, self.dist, self.comm = tok, device, group, dist, comm
        self.pack24 = bool(pack24)                # slab ids travel three bytes each (ids < 2**21): a quarter less on the links; EVERY rank alike
        _set_pack24(tok, self.pack24, self)
        if collective not in ("allgather", "p2p") or (collective == "p2p" and comm is None):
            raise ValueError("GatherV: collective is 'allgather' or -- with the library's communicator -- 'p2p'")
        self.collective = collective             # ncclAllGather of the bucket's slabs, or grouped send / recv of the same slabs
        self.world = comm.world if comm is not None else dist.get_world_size(group)
        self.depth = int(depth)
        self.max_docs = int(max_docs)
        self.max_tokens = int(max_tokens)
        self.cap_words = _slab_words(self.max_tokens, self.max_docs, self.pack24)
        if self.cap_words >= 1 << 32:
            raise ValueError("GatherV: a slab must stay below 2**32 words")
        self.off_stride = self.world * self.max_docs + 1
        self.ids_stride = self.world * self.max_tokens
        kw = dict(device=device)
        self.send = [torch.zeros(self.depth * self.cap_words, dtype=torch.int32, **kw) for _ in range(2)]
        self.recv = [torch.zeros(self.world * self.depth * self.cap_words, dtype=torch.int32, **kw) for _ in range(2)]
        # global CSR of each batch of the set's last exchanged bucket
        self.all_ids = [torch.zeros(self.depth * self.ids_stride, dtype=torch.int32, **kw) for _ in range(2)]
        self.all_off = [torch.zeros(self.depth * self.off_stride, dtype=torch.int64, **kw) for _ in range(2)]
        self.status = torch.zeros(1, dtype=torch.int32, **kw)
        self.exch = self._new_stream()
        self.packed = [self._new_event() for _ in range(2)]       # the bucket in set s is fully packed
        self.drained = [self._new_event() for _ in range(2)]      # the exchange of the bucket in set s is through
        self.in_flight = [False, False]
        self.cur, self.fill = 0, 0
        self.last = None                                          # (set, batches) of the last exchanged bucket
        self.on_bucket = None
        self._timing = None                                       # enable_timing(): [(start, end)] events per exchanged bucket

    # (overridable: the CPU test drives the bucket / event logic with a stub encoder on gloo)
    def _new_stream(self):
        return exchange_stream(self.dev)

    def _new_event(self):
        return torch.cuda.Event()

    def _main_stream(self):
        return torch.cuda.current_stream(self.dev)

    def _stream_ctx(self, st):
        return torch.cuda.stream(st)

    def enable_timing(self, on: bool = True) -> None:
        """Diagnostics for a scaling run: bracket every bucket's exchange (collective + unpack) with events on the
        exchange stream.  `exchange_ms()` then gives the time that stream spent in them -- beside the step time with
        and without the exchange that tells whether a rank is encode-bound or link-bound."""
        self._timing = [] if on else None

    def exchange_ms(self):
        """(total milliseconds, buckets) of the exchanges recorded since enable_timing(); synchronises."""
        if not self._timing:
            return 0.0, 0
        torch.cuda.synchronize(self.dev)
        total = sum(a.elapsed_time(b) for a, b in self._timing)
        n = len(self._timing)
        self._timing = []
        return float(total), n

    def bytes_per_bucket(self):
        """(bytes every rank SENDS per full bucket, bytes it RECEIVES): depth slabs of cap_words words out, world x that in."""
        sent = self.depth * self.cap_words * 4
        return sent, sent * self.world

    def _open_slab(self) -> torch.Tensor:
        main = self._main_stream()
        s = self.cur
        if self.fill == 0 and self.in_flight[s]:
            main.wait_event(self.drained[s])      # the set's previous exchange: normally long through
            self.in_flight[s] = False
        return self.send[s][self.fill * self.cap_words:(self.fill + 1) * self.cap_words]

    def _close_slab(self) -> None:
        self.fill += 1
        if self.fill == self.depth:
            self._exchange()

    def _pack(self, batch, slab, stream_ptr) -> None:
        _set_pack24(self.tok, self.pack24)
        rc = _ffi.lib().spl_gatherv_pack(self.tok.handle, batch.ids.data_ptr(), batch.out_off.data_ptr(), batch.n_docs,
                                         slab.data_ptr(), self.cap_words, self.max_docs, stream_ptr)
        if rc != 0:
            raise RuntimeError(_ffi.last_error())

    def _encode_packed(self, batch, slab, with_special, stream_ptr) -> None:
        _set_pack24(self.tok, self.pack24)
        rc = _ffi.lib().spl_encode_batch_device_packed(
            self.tok.handle, batch.text.data_ptr(), batch.n_bytes, batch.doc_off.data_ptr(), batch.n_docs,
            _ffi.SPL_WITH_SPECIAL if with_special else 0, batch.ids.data_ptr(), batch.ids.numel(),
            batch.out_off.data_ptr(), slab.data_ptr(), self.cap_words, self.max_docs, stream_ptr)
        if rc != 0:
            raise RuntimeError(f"spl_encode_batch_device_packed failed ({rc}): {_ffi.last_error()}")

    def _unpack(self, s, n, stream_ptr) -> None:
        rc = _ffi.lib().spl_gatherv_unpack_group(self.tok.handle, self.recv[s].data_ptr(), self.world, self.depth, n,
                                                 self.cap_words, self.max_docs, self.all_ids[s].data_ptr(),
                                                 self.ids_stride, self.all_off[s].data_ptr(), self.off_stride,
                                                 self.status.data_ptr(), stream_ptr)
        if rc != 0:
            raise RuntimeError(_ffi.last_error())

    def _allgather(self, s) -> None:
        """world x depth slabs, on the exchange stream (current here)."""
        if self.comm is not None:             # the collective behind the C ABI (librccl bound by the library)
            fn = _ffi.lib().spl_allgather_slabs_p2p if self.collective == "p2p" else _ffi.lib().spl_allgather_slabs
            rc = fn(self.comm.handle, self.send[s].data_ptr(), self.recv[s].data_ptr(), self.depth * self.cap_words, self.exch.cuda_stream)
            if rc != 0:
                raise RuntimeError(f"spl_allgather_slabs{'_p2p' if self.collective == 'p2p' else ''} failed ({rc}): {_ffi.last_error()}")
            return
        work = self.dist.all_gather_into_tensor(self.recv[s], self.send[s], group=self.group, async_op=True)
        work.wait()                           # the exchange stream (not the encode stream) waits for the collective

    def submit(self, batch: "DeviceBatch") -> None:
        """Pack `batch`'s current result into the open bucket (call right after encode_device on the
        same stream); a full bucket goes out."""
        slab = self._open_slab()
        self._pack(batch, slab, self._main_stream().cuda_stream)
        self._close_slab()

    def encode_and_submit(self, batch: "DeviceBatch", with_special: bool = False) -> None:
        """encode_device + submit in ONE call: the encoder's last kernel writes the slab itself
        (spl_encode_batch_device_packed), no separate pack launch."""
        slab = self._open_slab()
        self._encode_packed(batch, slab, with_special, self._main_stream().cuda_stream)
        self._close_slab()

    def _views(self, s, j):
        return (self.all_ids[s][j * self.ids_stride:(j + 1) * self.ids_stride],
                self.all_off[s][j * self.off_stride:(j + 1) * self.off_stride])

    def _exchange(self) -> None:
        main = self._main_stream()
        s, n = self.cur, self.fill
        self.packed[s].record(main)
        with self._stream_ctx(self.exch):
            self.exch.wait_event(self.packed[s])
            if self._timing is not None:
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record(self.exch)
            self._allgather(s)
            self._unpack(s, n, self.exch.cuda_stream)
            if self._timing is not None:
                ev[1].record(self.exch)
                self._timing.append(ev)
            if self.on_bucket is not None:
                self.on_bucket([self._views(s, j) for j in range(n)])
            self.drained[s].record(self.exch)
        self.in_flight[s] = True
        self.last = (s, n)
        self.cur ^= 1
        self.fill = 0

    def finish(self):
        """Flush and drain.  Returns (all_ids, all_off) of the LAST submitted batch: int32 ids (the
        first all_off[-1] entries are valid) and int64 offsets [world * max_docs + 1]."""
        if self.fill:
            self._exchange()
        main = self._main_stream()
        for s in (0, 1):
            if self.in_flight[s]:
                main.wait_event(self.drained[s])
                self.in_flight[s] = False
        if self.last is None:
            return self._views(0, 0)
        s, n = self.last
        return self._views(s, max(n - 1, 0))

    def overflowed(self) -> bool:
        return bool(self.status.item())


class WaveGather:
    """ONE batch, doc-sharded over the ranks (strong scaling), exchanged in WAVES so that the ids of wave k travel while wave k + 1 encodes.

    The batch's documents, in their order, are cut into `n_waves` waves and every wave into one contiguous slice per rank
    (splintr_amd.distributed.plan_waves); rank r encodes its slice of wave k straight into a slab (the encoder's last kernel writes it),
    an exchange stream of its own all-gathers the wave's `world` slabs and unpacks them BEHIND what the earlier waves left
    (spl_gatherv_unpack_at: running totals in device memory, advanced in stream order) -- no host synchronisation anywhere, the
    only exposed exchange is the last wave's.  After `finish()` every rank holds the CSR of the whole batch in document order.
    Order it replaces: Rayon's order-preserving collect, src/core/tokenizer.rs:932-942."""

    def __init__(self, tok: Tokenizer, device: torch.device, comm: "Comm", n_waves: int, max_docs: int, max_tokens: int,
                 total_tokens_cap: int, total_docs_cap: int, collective: str = "allgather", pack24: bool = False,
                 tok2: Optional[Tokenizer] = None, enc_pair: int = 0):
        self.tok, self.dev, self.comm, self.world = tok, device, comm, comm.world
        self.n_waves, self.max_docs, self.max_tokens = int(n_waves), int(max_docs), int(max_tokens)
        self.pack24 = bool(pack24)
        _set_pack24(tok, self.pack24, self)
        # A second handle of the same vocabulary (a workspace of its own): consecutive waves are then encoded on two streams in alternation,
        # wave k + 1's tile kernel starting while the stragglers of wave k's finish.  A rank's slice of a wave is small at high rank counts
        # (3.4 MB at 8 ranks x 8 waves), and launches of that size one after the other leave the GPU to every launch's ramp and tail: eight
        # of them took 0.90 ms on one stream, 0.69 ms on two -- one launch of the 27 MB: 0.63 (profiles/r05_wave_exchange.txt).
        self.toks = (tok,) if tok2 is None else (tok, tok2)
        if tok2 is not None:
            _set_pack24(tok2, self.pack24, self)
        self.enc = encode_streams(device, enc_pair) if tok2 is not None else None
        self.enc_pair = int(enc_pair)
        self.cap_words = _slab_words(self.max_tokens, self.max_docs, self.pack24)
        if self.cap_words >= 1 << 32:
            raise ValueError("WaveGather: a slab must stay below 2**32 words")
        self.collective = collective
        kw = dict(device=device)
        self.send = [torch.zeros(self.cap_words, dtype=torch.int32, **kw) for _ in range(self.n_waves)]
        self.recv = [torch.zeros(self.world * self.cap_words, dtype=torch.int32, **kw) for _ in range(self.n_waves)]
        self.all_ids = torch.zeros(int(total_tokens_cap), dtype=torch.int32, **kw)
        self.all_off = torch.zeros(int(total_docs_cap) + 1, dtype=torch.int64, **kw)
        self.run = torch.zeros(2, dtype=torch.int64, **kw)            # tokens, documents landed so far
        self.status = torch.zeros(1, dtype=torch.int32, **kw)
        self.exch = exchange_stream(device)
        self.encoded = [torch.cuda.Event() for _ in range(self.n_waves)]
        self.k = 0
        self._timing = None

    def enable_timing(self, on: bool = True) -> None:
        self._timing = [] if on else None

    def exchange_ms(self):
        if not self._timing:
            return 0.0, 0
        torch.cuda.synchronize(self.dev)
        total, n = sum(a.elapsed_time(b) for a, b in self._timing), len(self._timing)
        self._timing = []
        return float(total), n

    def _allgather(self, k) -> None:
        """wave k's `world` slabs, send[k] -> recv[k], on the exchange stream (current here).  (overridable: the GPU tests stand in for
        the other ranks of a world > 1 on one GPU)"""
        L = _ffi.lib()
        fn = L.spl_allgather_slabs_p2p if self.collective == "p2p" else L.spl_allgather_slabs
        rc = fn(self.comm.handle, self.send[k].data_ptr(), self.recv[k].data_ptr(), self.cap_words, self.exch.cuda_stream)
        if rc != 0:
            raise RuntimeError(f"spl_allgather_slabs failed ({rc}): {_ffi.last_error()}")

    def begin(self) -> None:
        """Start a new batch: the running totals back to zero (on the exchange stream, behind the previous batch's last unpack;
        the main stream waits for it only through finish())."""
        self.k = 0
        with torch.cuda.stream(self.exch):
            self.run.zero_()
        if self.enc is not None:                 # what the caller has queued so far (the batches' text) comes first
            main = torch.cuda.current_stream(self.dev)
            for st in self.enc:
                st.wait_stream(main)

    def encode_and_submit(self, batch: "DeviceBatch", with_special: bool = False) -> None:
        """This rank's slice of the next wave: encode (slab written by the encoder's last kernel) on the current stream, exchange and
        unpack on the exchange stream."""
        L = _ffi.lib()
        k = self.k
        main = torch.cuda.current_stream(self.dev) if self.enc is None else self.enc[k & 1]
        _set_pack24(self.toks[k % len(self.toks)], self.pack24)
        rc = L.spl_encode_batch_device_packed(self.toks[k % len(self.toks)].handle, batch.text.data_ptr(), batch.n_bytes, batch.doc_off.data_ptr(), batch.n_docs,
                                              _ffi.SPL_WITH_SPECIAL if with_special else 0, batch.ids.data_ptr(), batch.ids.numel(),
                                              batch.out_off.data_ptr(), self.send[k].data_ptr(), self.cap_words, self.max_docs, main.cuda_stream)
        if rc != 0:
            raise RuntimeError(f"spl_encode_batch_device_packed failed ({rc}): {_ffi.last_error()}")
        self.encoded[k].record(main)
        with torch.cuda.stream(self.exch):
            self.exch.wait_event(self.encoded[k])
            if self._timing is not None:
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record(self.exch)
            self._allgather(k)
            rc = L.spl_gatherv_unpack_at(self.tok.handle, self.recv[k].data_ptr(), self.world, self.cap_words, self.max_docs,
                                         self.all_ids.data_ptr(), self.all_ids.numel(), self.all_off.data_ptr(), self.all_off.numel(),
                                         self.run.data_ptr(), self.status.data_ptr(), self.exch.cuda_stream)
            if rc != 0:
                raise RuntimeError(f"spl_gatherv_unpack_at failed ({rc}): {_ffi.last_error()}")
            if self._timing is not None:
                ev[1].record(self.exch)
                self._timing.append(ev)
        self.k += 1

    def finish(self):
        """The main stream waits for the last wave's unpack.  Returns (all_ids, all_off, run): int32 ids, int64 offsets of the whole batch in
        document order, run = [total tokens, total documents] (device tensors; no host synchronisation here)."""
        torch.cuda.current_stream(self.dev).wait_stream(self.exch)
        return self.all_ids, self.all_off, self.run

    def overflowed(self) -> bool:
        return bool(self.status.item())
