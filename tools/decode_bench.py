#!/usr/bin/env python3
"""Time spl_decode_batch_device against the torch-op composition a user would otherwise write (GPU only).

The method is tools/collate_bench.py's: the two contenders produce IDENTICAL tensors (asserted with torch.equal) from the same
device-resident ids, and are timed in alternation in this one process -- a sample is a burst of back-to-back calls between two device
events on the current stream, the first rounds are warm-up.  Both allocate their outputs per call; a third line times the C-ABI call
into preallocated outputs (three launches, nothing else).  Printed per contender: the median over the bursts of the time per call, the
spread (max - min), the algorithmic bytes -- ids and offsets read, bytes and offsets written -- and their share of the HBM peak.

    python tools/decode_bench.py [--out profiles/decode_device.txt]

The composition: tok_len[ids], cumsum, repeat_interleave and a gather from the same id -> bytes table, the offsets by indexing; it is
GIVEN the output's size (repeat_interleave(output_size=...)), which a user would have to synchronise for.

Shapes: the C2 ids (corpus.c2(1000), cl100k_base), the C3 ids (corpus.c3(10000), o200k_base), rows [1000, 512] int64 from pad_device.
The bar: faster than the torch composition by more than the run-to-run spread (max - min) of the two together, on every shape.
The width of a lane's output group is a build-time constant (SPL_DEC_GROUP, 16 or 4); SPL_LIB_PATH selects a library built with the
other one, and the report names the library it measured."""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from collate_bench import bursts, report  # noqa: E402
from splintr_amd import Tokenizer, _ffi, corpus  # noqa: E402
from splintr_amd.device import DeviceBatch, decode_device, decode_reserve, decode_rows_device, encode_device, pad_device  # noqa: E402


def device_table(tok, dev):
    """id -> bytes of the vocabulary's dense range as torch tensors: start int64 [V + 1] and the blob"""
    L = _ffi.lib()
    p, n = ctypes.c_void_p(), ctypes.c_uint32()
    top = tok.vocab_size
    start, blob = np.zeros(top + 1, dtype=np.int64), bytearray()
    for i in range(top):
        if L.spl_token_bytes(tok.handle, i, ctypes.byref(p), ctypes.byref(n)):
            blob += ctypes.string_at(p, n.value)
        start[i + 1] = len(blob)
    return torch.from_numpy(start).to(dev), torch.from_numpy(np.frombuffer(bytes(blob), dtype=np.uint8).copy()).to(dev)


def torch_decode(ids, lens_tok, t_start, t_blob, doc_slot, total):
    """ids [T] (int64 indices), lens_tok [T]: each slot's byte count; doc_slot [n_docs + 1]: the slot every document starts at"""
    end = torch.cumsum(lens_tok, 0)
    beg = end - lens_tok
    owner = torch.repeat_interleave(torch.arange(ids.numel(), device=ids.device), lens_tok, output_size=total)
    src = t_start[ids][owner] + (torch.arange(total, device=ids.device) - beg[owner])
    out_off = torch.cat([end.new_zeros(1), end])[doc_slot]
    return t_blob[src], out_off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--seconds", type=float, default=0.4, help="device time per contender and shape")
    args = ap.parse_args()
    if not torch.cuda.is_available() or _ffi.lib().spl_device_count() == 0:
        sys.exit("decode_bench: no GPU")
    dev = torch.device("cuda", 0)
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    emit(f"decode_bench: {torch.cuda.get_device_name(0)}; library {os.path.basename(_ffi.LIB_PATH)}; per call, device events around bursts of "
         "back-to-back calls on one stream")
    L = _ffi.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    all_ok = True
    for label, vocab, texts, rows_shape in (("C2 corpus.c2(1000) cl100k_base", "cl100k_base", corpus.c2(1000), (1000, 512)),
                                            ("C3 corpus.c3(10000) o200k_base", "o200k_base", corpus.c3(10000), None)):
        tok = Tokenizer.from_pretrained(vocab)
        b = DeviceBatch(texts, dev)
        encode_device(tok, b)
        torch.cuda.synchronize()
        n, T = b.n_docs, int(b.out_off[-1].item())
        t_start, t_blob = device_table(tok, dev)
        t_len = t_start[1:] - t_start[:-1]
        decode_reserve(tok, max(b.ids.numel(), 1000 * 512))
        emit()
        emit(f"== {label}: {n} documents, {b.n_bytes} bytes, {T} tokens; longest token {L.spl_max_token_bytes(tok.handle)} bytes")
        # ---- CSR mode: the ids and offsets the encode left (ids.numel() = n_bytes is only an upper bound of the count)
        ids, off = b.ids, b.out_off
        total = b.n_bytes

        def composed():
            i = ids[:T].long()
            return torch_decode(i, t_len[i], t_start, t_blob, off, total)
        got, want = decode_device(tok, ids, off, max_bytes=total), composed()
        assert torch.equal(got[0][:total], want[0]) and torch.equal(got[1], want[1]), "CSR: the torch composition differs"
        assert want[0].cpu().numpy().tobytes() == b"".join(x.encode("utf-8") for x in texts)
        nbytes = 4 * T + 8 * (n + 1) + total + 8 * (n + 1)
        pre = [torch.empty_like(got[0]), torch.empty_like(got[1])]
        o = _ffi.SplDecodeOpts(0, 0)
        runs = {
            "spl decode_device": lambda: decode_device(tok, ids, off, max_bytes=total),
            "torch composition": composed,
            "spl_decode_batch_device prealloc": lambda: L.spl_decode_batch_device(tok.handle, ids.data_ptr(), ids.numel(), off.data_ptr(), None, n, ctypes.byref(o),
                                                                                  pre[0].data_ptr(), pre[0].numel(), pre[1].data_ptr(), st),
        }
        samples, inner = bursts(runs, args.seconds)
        all_ok &= report(emit, f"CSR  {T} ids in {n} documents -> {total} bytes", nbytes, samples, inner, "spl decode_device", "torch composition")
        assert torch.equal(pre[0][:total], want[0]) and torch.equal(pre[1], want[1])
        # ---- rows mode: [1000, 512] int64 from pad_device, with the lengths it returned
        if rows_shape:
            R, W = rows_shape
            rows, _, lens = pad_device(tok, b, W, pad_id=0, dtype=torch.int64)
            col = torch.arange(W, device=dev).unsqueeze(0)
            doc_slot = torch.arange(R + 1, device=dev) * W
            total_r = int(torch.where(col < lens.unsqueeze(1), t_len[rows], 0).sum().item())

            def composed_rows():
                valid = col < lens.unsqueeze(1)
                return torch_decode(rows.reshape(-1), torch.where(valid, t_len[rows], 0).reshape(-1), t_start, t_blob, doc_slot, total_r)
            got, want = decode_rows_device(tok, rows, lens, max_bytes=total_r), composed_rows()
            assert torch.equal(got[0][:total_r], want[0]) and torch.equal(got[1], want[1]), "rows: the torch composition differs"
            nbytes = 8 * R * W + 4 * R + total_r + 8 * (R + 1)
            pre = [torch.empty_like(got[0]), torch.empty_like(got[1])]
            o2 = _ffi.SplDecodeOpts(_ffi.SPL_DECODE_I64, W)
            runs = {
                "spl decode_rows_device": lambda: decode_rows_device(tok, rows, lens, max_bytes=total_r),
                "torch composition": composed_rows,
                "spl_decode_batch_device prealloc": lambda: L.spl_decode_batch_device(tok.handle, rows.data_ptr(), 0, None, lens.data_ptr(), R, ctypes.byref(o2),
                                                                                      pre[0].data_ptr(), pre[0].numel(), pre[1].data_ptr(), st),
            }
            samples, inner = bursts(runs, args.seconds)
            all_ok &= report(emit, f"rows [{R}, {W}] int64 + lengths -> {total_r} bytes", nbytes, samples, inner, "spl decode_rows_device", "torch composition")
            assert torch.equal(pre[0][:total_r], want[0]) and torch.equal(pre[1], want[1])
        del tok, b
    emit()
    emit("every shape faster than the torch composition by more than the spread: " + ("yes" if all_ok else "NO"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
