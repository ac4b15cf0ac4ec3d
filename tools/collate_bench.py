#!/usr/bin/env python3
"""Time spl_pad_device / spl_pack_device against the torch-op composition a user would otherwise write (GPU only).

For each shape and dtype the two contenders produce IDENTICAL tensors (asserted) from the same device-resident CSR, and are timed in
alternation in this one process: a sample is a burst of back-to-back calls between two device events on the current stream, bursts of
the two contenders take turns, the first rounds are warm-up.  Both allocate their outputs per call (torch's caching allocator), as a
user's code does; a third line times the C-ABI call into preallocated outputs -- the launch alone.  Printed per contender: the median
over the bursts of the time per call, the spread (min .. max, and p10 .. p90), the algorithmic bytes -- ids and offsets read plus
rows, mask and aux written, from the shapes -- and their share of the HBM peak at the median.

    python tools/collate_bench.py [--out profiles/collate.txt]

Shapes: the C2 batch (corpus.c2(1000), cl100k_base): pad L = 512, pack L = 2048; a C3-sized one (corpus.c3(10000), o200k_base): pad
L = 1024, pack L = 4096; int32 and int64 each.  The bar: faster than the torch composition by more than the run-to-run spread
(max - min) of the two together."""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from splintr_amd import Tokenizer, _ffi, corpus  # noqa: E402
from splintr_amd.device import DeviceBatch, encode_device, pack_device, pad_device  # noqa: E402

# MI355X, HBM3E: 8.0 TB/s specified; 6.29 TB/s is what a float4 copy kernel reaches (79 %)
HBM_PEAK = 8.0e12
HBM_COPY = 6.29e12
PAD_ID, BOS_ID, EOS_ID = 0, 1, 2


def torch_pad(ids, off, n_docs, L, dtype):
    """[BOS] head of the document [EOS], right-padded: the same tensors as pad_device(..., bos_id, eos_id)"""
    dev = ids.device
    lens = off[1:] - off[:-1]
    used = torch.clamp(lens, max=L - 2) + 2
    col = torch.arange(L, device=dev).unsqueeze(0)
    mask = col < used.unsqueeze(1)
    src = (off[:-1].unsqueeze(1) + col - 1).clamp_(0, ids.numel() - 1)
    rows = torch.where(mask, ids[src], PAD_ID)
    rows[:, 0] = BOS_ID
    rows.scatter_(1, (used - 1).unsqueeze(1), EOS_ID)
    return rows.to(dtype), mask.to(torch.uint8), used.to(torch.int32)


def torch_pack(ids, off, n_docs, L, rows_cap, dtype):
    """the stream of [BOS] ids [EOS] cut into rows_cap rows of L: the same tensors as pack_device(..., bos_id, eos_id, max_rows=rows_cap)"""
    dev = ids.device
    lens = off[1:] - off[:-1]
    starts = off[:-1] + 2 * torch.arange(n_docs, device=dev)
    S = off[-1] + 2 * n_docs
    p = torch.arange(rows_cap * L, device=dev)
    doc = torch.searchsorted(starts, p, right=True) - 1
    j = p - starts[doc]
    val = ids[(off[:-1][doc] + j - 1).clamp_(0, ids.numel() - 1)]
    val = torch.where(j == 0, BOS_ID, val)
    val = torch.where(j == lens[doc] + 1, EOS_ID, val)
    live = p < S
    rows = torch.where(live, val, PAD_ID).to(dtype).view(rows_cap, L)
    docs = torch.where(live, doc, -1).to(torch.int32).view(rows_cap, L)
    pos = torch.where(live, torch.minimum(j, p % L), 0).to(torch.int32).view(rows_cap, L)
    n = torch.stack([(S + L - 1) // L, S])
    return rows, docs, pos, n


def bursts(contenders, seconds, rounds=21, warm=3):
    """{name: [ms per call, one per burst]}: bursts of the contenders in alternation, each burst long enough to time"""
    inner = {}
    for name, fn in contenders.items():          # size a burst: about seconds / rounds of device time
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        torch.cuda.synchronize()
        a.record()
        for _ in range(5):
            fn()
        b.record()
        torch.cuda.synchronize()
        inner[name] = max(3, int(seconds / rounds / max(a.elapsed_time(b) / 5e3, 1e-7)))
    out = {name: [] for name in contenders}
    for r in range(warm + rounds):
        for name, fn in contenders.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner[name]):
                fn()
            b.record()
            torch.cuda.synchronize()
            if r >= warm:
                out[name].append(a.elapsed_time(b) / inner[name])
    return out, inner


def report(emit, title, nbytes, samples, inner, ours, base):
    emit(f"{title}   algorithmic bytes {nbytes / 1e6:.2f} MB")
    stat = {}
    for name, xs in samples.items():
        s = sorted(xs)
        med, lo, hi = s[len(s) // 2], s[0], s[-1]
        p10, p90 = s[len(s) // 10], s[-1 - len(s) // 10]
        stat[name] = (med, hi - lo)
        bw = nbytes / (med * 1e-3)
        emit(f"  {name:<28} median {med * 1e3:9.2f} us   min {lo * 1e3:9.2f}  max {hi * 1e3:9.2f}  p10-p90 {p10 * 1e3:9.2f} .. {p90 * 1e3:9.2f} us"
             f"   {bw / 1e9:8.1f} GB/s = {100 * bw / HBM_PEAK:5.1f} % of 8.0 TB/s ({100 * bw / HBM_COPY:5.1f} % of a copy's 6.29)   [{len(s)} bursts x {inner[name]} calls]")
    gain, spread = stat[base][0] - stat[ours][0], stat[base][1] + stat[ours][1]
    ok = gain > spread
    emit(f"  -> {ours} is {stat[base][0] / stat[ours][0]:.2f}x the torch composition; gain {gain * 1e3:.2f} us against a spread (max - min, both) of "
         f"{spread * 1e3:.2f} us: {'PASS' if ok else 'MISS'}")
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--seconds", type=float, default=0.4, help="device time per contender and shape")
    args = ap.parse_args()
    if not torch.cuda.is_available() or _ffi.lib().spl_device_count() == 0:
        sys.exit("collate_bench: no GPU")
    dev = torch.device("cuda", 0)
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    emit(f"collate_bench: {torch.cuda.get_device_name(0)}; per call, device events around bursts of back-to-back calls on one stream")
    all_ok = True
    for label, vocab, texts, L_pad, L_pack in (("C2 corpus.c2(1000) cl100k_base", "cl100k_base", corpus.c2(1000), 512, 2048),
                                               ("C3 corpus.c3(10000) o200k_base", "o200k_base", corpus.c3(10000), 1024, 4096)):
        tok = Tokenizer.from_pretrained(vocab)
        b = DeviceBatch(texts, dev)
        encode_device(tok, b)
        torch.cuda.synchronize()
        n, T = b.n_docs, int(b.out_off[-1].item())
        ids, off = b.ids, b.out_off
        S = T + 2 * n
        cap = (S + L_pack - 1) // L_pack
        emit()
        emit(f"== {label}: {n} documents, {b.n_bytes} bytes, {T} tokens")
        L = _ffi.lib()
        st = torch.cuda.current_stream(dev).cuda_stream
        for dtype, isz, name in ((torch.int32, 4, "int32"), (torch.int64, 8, "int64")):
            fl = (_ffi.SPL_COLLATE_I64 if isz == 8 else 0) | _ffi.SPL_COLLATE_BOS | _ffi.SPL_COLLATE_EOS
            # ---- pad
            got = pad_device(tok, b, L_pad, pad_id=PAD_ID, bos_id=BOS_ID, eos_id=EOS_ID, dtype=dtype)
            want = torch_pad(ids, off, n, L_pad, dtype)
            assert all(torch.equal(g, w) for g, w in zip(got, want)), "pad: the torch composition differs"
            kept = int(want[2].sum().item()) - 2 * n
            nbytes = 4 * kept + 8 * (n + 1) + n * L_pad * (isz + 1) + 4 * n
            o = _ffi.SplCollateOpts(fl, L_pad, PAD_ID, BOS_ID, EOS_ID)
            pre = [torch.empty_like(t) for t in got]
            runs = {
                "spl pad_device": lambda: pad_device(tok, b, L_pad, pad_id=PAD_ID, bos_id=BOS_ID, eos_id=EOS_ID, dtype=dtype),
                "torch composition": lambda: torch_pad(ids, off, n, L_pad, dtype),
                "spl_pad_device preallocated": lambda: L.spl_pad_device(tok.handle, ids.data_ptr(), off.data_ptr(), n, ctypes.byref(o), pre[0].data_ptr(),
                                                                        pre[1].data_ptr(), pre[2].data_ptr(), st),
            }
            samples, inner = bursts(runs, args.seconds)
            all_ok &= report(emit, f"pad  [{n}, {L_pad}] {name} + mask + lengths", nbytes, samples, inner, "spl pad_device", "torch composition")
            assert all(torch.equal(g, w) for g, w in zip(pre, want))
            # ---- pack
            got = pack_device(tok, b, L_pack, pad_id=PAD_ID, bos_id=BOS_ID, eos_id=EOS_ID, dtype=dtype, max_rows=cap)
            want = torch_pack(ids, off, n, L_pack, cap, dtype)
            assert all(torch.equal(g, w) for g, w in zip(got, want)), "pack: the torch composition differs"
            nbytes = 4 * T + 8 * (n + 1) + cap * L_pack * (isz + 8) + 16
            pre = [torch.empty_like(t) for t in got]
            o2 = _ffi.SplCollateOpts(fl, L_pack, PAD_ID, BOS_ID, EOS_ID)
            runs = {
                "spl pack_device": lambda: pack_device(tok, b, L_pack, pad_id=PAD_ID, bos_id=BOS_ID, eos_id=EOS_ID, dtype=dtype, max_rows=cap),
                "torch composition": lambda: torch_pack(ids, off, n, L_pack, cap, dtype),
                "spl_pack_device preallocated": lambda: L.spl_pack_device(tok.handle, ids.data_ptr(), off.data_ptr(), n, ctypes.byref(o2), pre[0].data_ptr(), cap,
                                                                          pre[1].data_ptr(), pre[2].data_ptr(), pre[3].data_ptr(), st),
            }
            samples, inner = bursts(runs, args.seconds)
            all_ok &= report(emit, f"pack [{cap}, {L_pack}] {name} + doc_ids + positions", nbytes, samples, inner, "spl pack_device", "torch composition")
            assert all(torch.equal(g, w) for g, w in zip(pre, want))
        del tok, b
    emit()
    emit("every shape faster than the torch composition by more than the spread: " + ("yes" if all_ok else "NO"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
