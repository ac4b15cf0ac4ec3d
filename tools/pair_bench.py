#!/usr/bin/env python3
"""Time spl_pair_device against the torch-op composition a user would otherwise write, and against joining the strings (GPU only).

Method as tools/collate_bench.py (its bursts / report are used): the contenders produce IDENTICAL tensors (asserted once, before any
timing) from the same device-resident encode result and are timed in alternation in this one process -- a sample is a burst of
back-to-back calls between two device events on the current stream, the median over the bursts is reported with its spread.

    python tools/pair_bench.py [--out profiles/pairs.txt]

Cases, all in BERT's form [CLS] a [SEP] b [SEP], longest_first, heads kept, padding on the right:
  one query    a ~30-token query as A (ONE document, named by a_index = zeros) against corpus.c2(1000) as B; rows of 512, int32 and
               int64.  Also (b): the existing route -- the 1000 JOINED strings encoded and padded (encode_device + pad_device) -- against
               this one's whole cost (encode_device of 1 + 1000 texts + pair_device).  Time only: (b)'s ids differ at the seam by design.
  one to one   10 000 short queries paired with corpus.c3(10000), rows of 1024, int32 and int64.
Lines per case: pair_device (allocates its outputs per call, as the composition does), the torch composition, spl_pair_device alone
(the C-ABI call into preallocated outputs: the launch)."""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from collate_bench import bursts, report  # noqa: E402
from splintr_amd import Tokenizer, _ffi, corpus  # noqa: E402
from splintr_amd.device import DeviceBatch, encode_device, pad_device, pair_csr_device  # noqa: E402

PAD_ID, CLS, SEP = 0, 101, 102
QUERY = ("which of these passages explains how a byte pair encoding tokenizer decides where one token ends and the next one begins, "
         "and what happens at the boundary between two texts?")


def torch_pair(ids, a_off, n_a, b_off, n_b, a_idx, b_idx, n_pairs, L, dtype):
    """[CLS] A' [SEP] B' [SEP] right-padded, longest_first with the heads kept: the same seven tensors as pair_csr_device(...,
    prefix=[CLS], middle=[SEP], suffix=[SEP]) for indices that all name a document"""
    dev = ids.device
    ia = torch.arange(n_pairs, device=dev) if a_idx is None else a_idx.long()
    ib = torch.arange(n_pairs, device=dev) if b_idx is None else b_idx.long()
    a0, b0 = a_off[:n_a][ia], b_off[:n_b][ib]
    la, lb = a_off[1:n_a + 1][ia] - a0, b_off[1:n_b + 1][ib] - b0
    B = L - 3
    hB = B // 2
    hA = B - hB
    fits, short_a, short_b = la + lb <= B, la < hA, lb <= hB
    na = torch.where(fits | short_a, la, torch.where(short_b, B - lb, hA))
    nb = torch.where(fits, lb, torch.where(short_a, B - la, torch.where(short_b, lb, hB)))
    col = torch.arange(L, device=dev).unsqueeze(0)
    e2, e3 = (1 + na).unsqueeze(1), (2 + na).unsqueeze(1)
    e4 = e3 + nb.unsqueeze(1)
    used = e4 + 1
    in_a, in_b = (col >= 1) & (col < e2), (col >= e3) & (col < e4)
    src = torch.where(in_a, a0.unsqueeze(1) + col - 1, b0.unsqueeze(1) + col - e3).clamp_(0, ids.numel() - 1)
    rows = torch.where(in_a | in_b, ids[src], PAD_ID)
    rows[:, 0] = CLS
    rows = torch.where((col == e2) | (col == e4), SEP, rows)
    mask = col < used
    return (rows.to(dtype), mask.to(torch.uint8), ((col >= e3) & mask).to(torch.uint8), (~(in_a | in_b)).to(torch.uint8),
            used.squeeze(1).to(torch.int32), torch.stack([na, nb], dim=1).to(torch.int32), torch.zeros(1, dtype=torch.int32, device=dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--seconds", type=float, default=0.4, help="device time per contender and shape")
    args = ap.parse_args()
    if not torch.cuda.is_available() or _ffi.lib().spl_device_count() == 0:
        sys.exit("pair_bench: no GPU")
    dev = torch.device("cuda", 0)
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    emit(f"pair_bench: {torch.cuda.get_device_name(0)}; per call, device events around bursts of back-to-back calls on one stream")
    L = _ffi.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    faster = True
    cases = (("one query x C2 corpus.c2(1000) cl100k_base", "cl100k_base", [QUERY], corpus.c2(1000), 512, True),
             ("10000 queries 1:1 C3 corpus.c3(10000) o200k_base", "o200k_base",
              [f"query {i}: what does passage {i} say about item {i * 7919 % 10007}?" for i in range(10000)], corpus.c3(10000), 1024, False))
    for label, vocab, a_texts, b_texts, row_len, one_query in cases:
        tok = Tokenizer.from_pretrained(vocab)
        b = DeviceBatch(a_texts + b_texts, dev)
        encode_device(tok, b)
        torch.cuda.synchronize()
        n_a, n_b = len(a_texts), len(b_texts)
        n_pairs = n_b
        ids, a_off, b_off = b.ids, b.out_off, b.out_off[n_a:]
        a_idx = torch.zeros(n_pairs, dtype=torch.int32, device=dev) if one_query else None
        off = b.out_off.cpu()
        emit()
        emit(f"== {label}: A {n_a} documents, {int(off[n_a])} tokens; B {n_b} documents, {int(off[-1] - off[n_a])} tokens; {n_pairs} pairs")
        for dtype, isz, name in ((torch.int32, 4, "int32"), (torch.int64, 8, "int64")):
            kw = dict(pad_id=PAD_ID, prefix=[CLS], middle=[SEP], suffix=[SEP], a_index=a_idx, dtype=dtype)
            call = lambda: pair_csr_device(tok, ids, a_off, n_a, ids, b_off, n_b, row_len, **kw)
            got = call()
            want = torch_pair(ids, a_off, n_a, b_off, n_b, a_idx, None, n_pairs, row_len, dtype)
            assert all(torch.equal(g, w) for g, w in zip(got, want)), "the torch composition differs"
            kept = int(want[5].sum().item())
            nbytes = 4 * kept + 16 * n_pairs + (4 * n_pairs if one_query else 0) + n_pairs * row_len * (isz + 3) + 12 * n_pairs
            o = _ffi.SplPairOpts((_ffi.SPL_COLLATE_I64 if isz == 8 else 0), row_len, PAD_ID, _ffi.SPL_PAIR_LONGEST_FIRST, [CLS], [SEP], [SEP])
            pre = [torch.empty_like(t) for t in got[:6]] + [torch.zeros_like(got[6])]
            runs = {
                "spl pair_device": call,
                "torch composition": lambda: torch_pair(ids, a_off, n_a, b_off, n_b, a_idx, None, n_pairs, row_len, dtype),
                "spl_pair_device preallocated": lambda: L.spl_pair_device(
                    tok.handle, ids.data_ptr(), a_off.data_ptr(), n_a, ids.data_ptr(), b_off.data_ptr(), n_b,
                    a_idx.data_ptr() if a_idx is not None else None, None, n_pairs, ctypes.byref(o), pre[0].data_ptr(), pre[1].data_ptr(),
                    pre[2].data_ptr(), pre[3].data_ptr(), pre[4].data_ptr(), pre[5].data_ptr(), pre[6].data_ptr(), st),
            }
            samples, inner = bursts(runs, args.seconds)
            faster &= report(emit, f"pair [{n_pairs}, {row_len}] {name} + mask + types + special + lengths + kept", nbytes, samples, inner,
                             "spl pair_device", "torch composition")
            assert all(torch.equal(g, w) for g, w in zip(pre, want))
        if one_query:
            # (b) the existing route: join the strings, encode the 1000 joined texts, pad_device -- against this route's whole cost
            joined = DeviceBatch([a_texts[0] + " " + t for t in b_texts], dev)
            runs = {
                "joined strings: encode + pad_device": lambda: (encode_device(tok, joined),
                                                                pad_device(tok, joined, row_len, pad_id=PAD_ID, bos_id=CLS, eos_id=SEP)),
                "pairs: encode once + pair_device": lambda: (encode_device(tok, b),
                                                             pair_csr_device(tok, ids, a_off, n_a, ids, b_off, n_b, row_len, pad_id=PAD_ID,
                                                                             prefix=[CLS], middle=[SEP], suffix=[SEP], a_index=a_idx)),
            }
            samples, inner = bursts(runs, args.seconds)
            emit(f"(b) the whole route, texts already on the device: {joined.n_bytes} bytes joined against {b.n_bytes} bytes separate "
                 "(time only: the joined route's ids differ at the seam by design)")
            for nm, xs in samples.items():
                s = sorted(xs)
                emit(f"  {nm:<38} median {s[len(s) // 2] * 1e3:9.2f} us   min {s[0] * 1e3:9.2f}  max {s[-1] * 1e3:9.2f}   [{len(s)} bursts x {inner[nm]} calls]")
        del tok, b
    emit()
    emit("every shape faster than the torch composition by more than the spread: " + ("yes" if faster else "NO"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
