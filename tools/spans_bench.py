#!/usr/bin/env python3
"""Time spl_token_spans_device against the torch-op composition a user would otherwise write (GPU only).

The method is tools/collate_bench.py's: the two contenders produce IDENTICAL tensors (asserted with torch.equal) from the same
device-resident ids, and are timed in alternation in this one process -- a sample is a burst of back-to-back calls between two device
events on the current stream, 21 bursts after 3 warm-up rounds.  Both allocate their outputs per call; a third line times the C-ABI
call into preallocated outputs (four launches, nothing else).  Printed per contender: the median over the bursts of the time per call,
the spread (max - min), the algorithmic bytes -- ids and offsets read, two span arrays and two offset arrays written -- and their share
of the HBM peak.

    python tools/spans_bench.py [--out profiles/spans.txt]

The composition: three table lookups (byte length, characters, continuation flag per id), two cumsums, searchsorted for every slot's
document, the subtraction of the document's start sums, the continuation adjustment, the offsets by indexing.

Shapes: the C2 ids (corpus.c2(1000), cl100k_base) and the C3 ids (corpus.c3(10000), o200k_base), as the encode leaves them (the id
buffer's capacity is the text's byte count: the slots behind the token count belong to no document).
The bar: faster than the torch composition by more than the run-to-run spread (max - min) of the two together, on every shape.
Control in the same run: decode_device on the C2 ids (code this tool's subject does not touch)."""
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
from splintr_amd.device import DeviceBatch, decode_device, decode_reserve, encode_device  # noqa: E402


def device_tables(tok, dev):
    """per id of the vocabulary's range, as int64 tensors: byte length, bytes that start a character, first byte is a continuation"""
    L = _ffi.lib()
    p, n = ctypes.c_void_p(), ctypes.c_uint32()
    top = tok.vocab_size
    ln, nch, cont = (np.zeros(top, dtype=np.int64) for _ in range(3))
    for i in range(top):
        if L.spl_token_bytes(tok.handle, i, ctypes.byref(p), ctypes.byref(n)) and n.value:
            b = np.frombuffer(ctypes.string_at(p, n.value), dtype=np.uint8)
            ln[i], nch[i], cont[i] = len(b), int(((b & 0xC0) != 0x80).sum()), int((b[0] & 0xC0) == 0x80)
    return tuple(torch.from_numpy(x).to(dev) for x in (ln, nch, cont))


def torch_spans(ids, off, T, t_len, t_nch, t_cont):
    """the tensors spans_device returns, from torch ops; T (the token count) is GIVEN: a user would have to synchronise for it"""
    dev = ids.device
    i = ids[:T].long()
    ln, nc, ct = t_len[i], t_nch[i], t_cont[i]
    gb = torch.cat([ln.new_zeros(1), torch.cumsum(ln, 0)])
    gc = torch.cat([nc.new_zeros(1), torch.cumsum(nc, 0)])
    doc = torch.searchsorted(off, torch.arange(T, device=dev), right=True) - 1
    start = off[doc]
    bs = gb[:T] - gb[start]
    cs = gc[:T] - gc[start]
    byte_span = torch.zeros(ids.numel(), 2, dtype=torch.int32, device=dev)
    char_span = torch.zeros(ids.numel(), 2, dtype=torch.int32, device=dev)
    byte_span[:T] = torch.stack([bs, bs + ln], 1)
    char_span[:T] = torch.stack([cs - (ct & (cs > 0)), cs + nc], 1)
    return byte_span, char_span, gb[off], gc[off]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--seconds", type=float, default=0.4, help="device time per contender and shape")
    args = ap.parse_args()
    if not torch.cuda.is_available() or _ffi.lib().spl_device_count() == 0:
        sys.exit("spans_bench: no GPU")
    from splintr_amd.device import spans_device
    dev = torch.device("cuda", 0)
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    emit(f"spans_bench: {torch.cuda.get_device_name(0)}; library {os.path.basename(_ffi.LIB_PATH)}; per call, device events around bursts of "
         "back-to-back calls on one stream")
    L = _ffi.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    all_ok = True
    for label, vocab, texts in (("C2 corpus.c2(1000) cl100k_base", "cl100k_base", corpus.c2(1000)),
                                ("C3 corpus.c3(10000) o200k_base", "o200k_base", corpus.c3(10000))):
        tok = Tokenizer.from_pretrained(vocab)
        b = DeviceBatch(texts, dev)
        encode_device(tok, b)
        torch.cuda.synchronize()
        n, T = b.n_docs, int(b.out_off[-1].item())
        t_len, t_nch, t_cont = device_tables(tok, dev)
        decode_reserve(tok, b.ids.numel())
        ids, off = b.ids, b.out_off
        emit()
        emit(f"== {label}: {n} documents, {b.n_bytes} bytes, {T} tokens in {ids.numel()} slots")

        def composed():
            return torch_spans(ids, off, T, t_len, t_nch, t_cont)
        got, want = spans_device(tok, ids, off), composed()
        for g, w, what in zip(got, want, ("byte_span", "char_span", "byte_off", "char_off")):
            assert torch.equal(g, w), f"the torch composition differs: {what}"
        assert got[2].cpu().tolist() == b.host_offsets.tolist()
        nbytes = 4 * T + 8 * (n + 1) + 2 * 8 * ids.numel() + 2 * 8 * (n + 1)
        pre = [torch.empty_like(x) for x in got]
        o = _ffi.SplDecodeOpts(0, 0)
        runs = {
            "spl spans_device": lambda: spans_device(tok, ids, off),
            "torch composition": composed,
            "spl_token_spans_device prealloc": lambda: L.spl_token_spans_device(tok.handle, ids.data_ptr(), ids.numel(), off.data_ptr(), None, n, ctypes.byref(o), 0,
                                                                                pre[0].data_ptr(), pre[1].data_ptr(), pre[2].data_ptr(), pre[3].data_ptr(), st),
        }
        if vocab == "cl100k_base":             # the control: code the spans do not touch, in the same alternation
            runs["control: spl decode_device"] = lambda: decode_device(tok, ids, off, max_bytes=b.n_bytes)
        samples, inner = bursts(runs, args.seconds)
        all_ok &= report(emit, f"CSR  {T} ids in {n} documents", nbytes, samples, inner, "spl spans_device", "torch composition")
        for g, w in zip(pre, want):
            assert torch.equal(g, w)
        del tok, b
    emit()
    emit("every shape faster than the torch composition by more than the spread: " + ("yes" if all_ok else "NO"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
