#!/usr/bin/env python3
"""Time spl_window_device against the torch-op composition a user would otherwise write (GPU only); tools/collate_bench.py's method.

For each shape and dtype the contenders produce IDENTICAL tensors (asserted with torch.equal) from the same device-resident CSR and are
timed in alternation in this one process: bursts of back-to-back calls between two device events, the first rounds warm-up; median and
spread per contender.  Lines per shape: window_device as a user calls it (outputs allocated per call), the torch composition, the C-ABI
call into preallocated outputs (the launches alone: scan + gather), and the same call with rows_cap = 0 (the scan's launches alone; the
gather's share is the difference of the two medians).  Algorithmic bytes come from the shapes: ids read (a window's body each), offsets
read, row offsets written and read, rows + mask + the per-row arrays written.

    python tools/window_bench.py [--out profiles/window.txt]

Shapes: C2 (corpus.c2(1000), cl100k_base), L = 128, overlap 16; C3 (corpus.c3(10000), o200k_base), L = 512, overlap 64; int32 and
int64 each, BOS and EOS on.  The bar is collate_bench's: faster than the torch composition by more than the run-to-run spread (max - min)
of the two together.  As a control one pad and one pack shape of profiles/collate.txt are measured again in the same run."""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from collate_bench import BOS_ID, EOS_ID, PAD_ID, bursts, report, torch_pack, torch_pad  # noqa: E402


def torch_window(ids, off, n_docs, L, overlap, rows_cap, dtype):
    """windows of [BOS] body [EOS], right-padded, rows_cap rows: the same tensors as window_device(..., bos_id, eos_id, max_rows=rows_cap)"""
    dev = ids.device
    B = L - 2
    step = B - overlap
    lens = off[1:] - off[:-1]
    n_w = 1 + torch.clamp(torch.div(lens - B + step - 1, step, rounding_mode="floor"), min=0)
    row_off = torch.zeros(n_docs + 1, dtype=torch.int64, device=dev)
    torch.cumsum(n_w, 0, out=row_off[1:])
    R = row_off[-1]
    r = torch.arange(rows_cap, device=dev)
    live = r < R
    doc = torch.searchsorted(row_off[1:], r, right=True).clamp_(max=n_docs - 1)
    start = (r - row_off[doc]) * step
    v0 = off[doc] + start
    used = torch.where(live, torch.clamp(off[doc + 1] - v0, max=B) + 2, 1)
    col = torch.arange(L, device=dev).unsqueeze(0)
    mask = (col < used.unsqueeze(1)) & live.unsqueeze(1)
    src = (v0.unsqueeze(1) + col - 1).clamp_(0, ids.numel() - 1)
    rows = torch.where(mask, ids[src], PAD_ID)
    rows[:, 0] = torch.where(live, BOS_ID, PAD_ID)
    rows.scatter_(1, (used - 1).unsqueeze(1), torch.where(live, EOS_ID, PAD_ID).to(rows.dtype).unsqueeze(1))
    n = torch.stack([R, torch.clamp(R, max=rows_cap)])
    return (rows.to(dtype), mask.to(torch.uint8), torch.where(live, used, 0).to(torch.int32), torch.where(live, doc, -1).to(torch.int32),
            torch.where(live, start, 0), row_off, n)


def main():
    from splintr_amd import Tokenizer, _ffi, corpus
    from splintr_amd.device import DeviceBatch, encode_device, pack_device, pad_device, window_device
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--seconds", type=float, default=0.4, help="device time per contender and shape")
    args = ap.parse_args()
    if not torch.cuda.is_available() or _ffi.lib().spl_device_count() == 0:
        sys.exit("window_bench: no GPU")
    dev = torch.device("cuda", 0)
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    emit(f"window_bench: {torch.cuda.get_device_name(0)}; per call, device events around bursts of back-to-back calls on one stream")
    lib = _ffi.lib()
    all_ok = True
    for label, vocab, texts, L, overlap in (("C2 corpus.c2(1000) cl100k_base", "cl100k_base", corpus.c2(1000), 128, 16),
                                            ("C3 corpus.c3(10000) o200k_base", "o200k_base", corpus.c3(10000), 512, 64)):
        tok = Tokenizer.from_pretrained(vocab)
        b = DeviceBatch(texts, dev)
        encode_device(tok, b)
        torch.cuda.synchronize()
        n, T = b.n_docs, int(b.out_off[-1].item())
        ids, off = b.ids, b.out_off
        st = torch.cuda.current_stream(dev).cuda_stream
        probe = window_device(tok, b, L, overlap=overlap, pad_id=PAD_ID, bos_id=BOS_ID, eos_id=EOS_ID)
        cap = int(probe[6][0].item())                 # exactly the rows the batch needs
        spans = -(-n // 4096)
        emit()
        emit(f"== {label}: {n} documents, {b.n_bytes} bytes, {T} tokens; L = {L}, overlap {overlap}: {cap} rows ({cap / n:.2f} per document); "
             f"launches: scan {1 if spans <= 1 else 3} + gather 1, workspace {lib.spl_window_work_bytes(n)} bytes")
        del probe
        for dtype, isz, name in ((torch.int32, 4, "int32"), (torch.int64, 8, "int64")):
            fl = (_ffi.SPL_COLLATE_I64 if isz == 8 else 0) | _ffi.SPL_COLLATE_BOS | _ffi.SPL_COLLATE_EOS
            got = window_device(tok, b, L, overlap=overlap, pad_id=PAD_ID, bos_id=BOS_ID, eos_id=EOS_ID, dtype=dtype, max_rows=cap)
            want = torch_window(ids, off, n, L, overlap, cap, dtype)
            assert all(torch.equal(g, w) for g, w in zip(got, want)), "window: the torch composition differs"
            body = int(want[2].sum().item()) - 2 * cap
            nbytes = 4 * body + 8 * (n + 1) + 2 * 8 * (n + 1) + cap * L * (isz + 1) + cap * 16 + 16
            o = _ffi.SplCollateOpts(fl, L, PAD_ID, BOS_ID, EOS_ID)
            pre = [torch.empty_like(t) for t in got]
            work = torch.empty(max(int(lib.spl_window_work_bytes(n)), 8), dtype=torch.uint8, device=dev)

            def abi(rows_cap):
                return lib.spl_window_device(tok.handle, ids.data_ptr(), off.data_ptr(), n, ctypes.byref(o), overlap, pre[0].data_ptr(), rows_cap,
                                             pre[1].data_ptr(), pre[2].data_ptr(), pre[3].data_ptr(), pre[4].data_ptr(), pre[5].data_ptr(),
                                             pre[6].data_ptr(), work.data_ptr(), st)
            runs = {
                "spl window_device": lambda: window_device(tok, b, L, overlap=overlap, pad_id=PAD_ID, bos_id=BOS_ID, eos_id=EOS_ID, dtype=dtype, max_rows=cap),
                "torch composition": lambda: torch_window(ids, off, n, L, overlap, cap, dtype),
                "spl_window_device prealloc.": lambda: abi(cap),
                "... rows_cap 0: the scan alone": lambda: abi(0),
            }
            samples, inner = bursts(runs, args.seconds)
            all_ok &= report(emit, f"window [{cap}, {L}] {name} + mask + lengths + doc + start + row_off", nbytes, samples, inner,
                             "spl window_device", "torch composition")
            med = {k: sorted(v)[len(v) // 2] for k, v in samples.items()}
            emit(f"  (the gather's share: {1e3 * (med['spl_window_device prealloc.'] - med['... rows_cap 0: the scan alone']):.2f} us = preallocated call - scan alone; "
                 f"the scan's line moves {8 * (n + 1) * 2 / 1e3:.1f} KB, not the bytes above)")
            assert abi(cap) == 0
            assert all(torch.equal(g, w) for g, w in zip(pre, want))
        if label.startswith("C2"):                    # the control: pad and pack compile from unchanged code (profiles/collate.txt)
            for kind, Lc in (("pad", 512), ("pack", 2048)):
                if kind == "pad":
                    ours, theirs = (lambda: pad_device(tok, b, Lc, pad_id=PAD_ID, bos_id=BOS_ID, eos_id=EOS_ID)), (lambda: torch_pad(ids, off, n, Lc, torch.int32))
                    kept = int(theirs()[2].sum().item()) - 2 * n
                    nbytes = 4 * kept + 8 * (n + 1) + n * Lc * 5 + 4 * n
                else:
                    capk = (T + 2 * n + Lc - 1) // Lc
                    ours = lambda: pack_device(tok, b, Lc, pad_id=PAD_ID, bos_id=BOS_ID, eos_id=EOS_ID, max_rows=capk)      # noqa: E731
                    theirs = lambda: torch_pack(ids, off, n, Lc, capk, torch.int32)                                        # noqa: E731
                    nbytes = 4 * T + 8 * (n + 1) + capk * Lc * 12 + 16
                assert all(torch.equal(g, w) for g, w in zip(ours(), theirs()))
                samples, inner = bursts({f"spl {kind}_device": ours, "torch composition": theirs}, args.seconds)
                report(emit, f"control: {kind} C2 L = {Lc} int32 (compare profiles/collate.txt)", nbytes, samples, inner, f"spl {kind}_device", "torch composition")
        del tok, b
    emit()
    emit("every window shape faster than the torch composition by more than the spread: " + ("yes" if all_ok else "NO"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
