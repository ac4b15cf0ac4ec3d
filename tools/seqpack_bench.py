#!/usr/bin/env python3
"""Time spl_seqpack_device (whole-sequence packing) and, for next_fit, the composition a user would otherwise write (GPU only).

Method as tools/collate_bench.py (its bursts / report are used): contenders are timed in alternation in this one process -- a sample is a
burst of back-to-back calls between two device events on the current stream, the median over the bursts is reported with its spread.

    python tools/seqpack_bench.py [--out profiles/seqpack.txt]

Input: tools/chat_bench.py's conversations as chat_device leaves them (input_ids, labels, loss_mask, role_ids, special_tokens_mask,
lengths), packed into rows of the same length:
  C2   250 conversations, rows [250, 2048], int32 and int64
  C3   2500 conversations, rows [2500, 8192], int32 and int64
each packed into rows of the input's length (chat_bench's shapes: what fits is what two conversations of ~1 150 / ~5 000 ids allow) and of
TWICE that length.
Per shape and strategy: seqpack_rows_device (allocates its outputs per call), spl_seqpack_device into preallocated outputs (the two
launches alone), the same with max_rows = 0 (the PLAN launch alone: no gather is launched), and COUNTS: rows needed and the padding
share before and after packing.  For next_fit the composition: the lengths to the host, the reference's loop in Python, the plan back to the
device, torch index ops for input_ids, labels and position_ids -- asserted equal (torch.equal) before any timing."""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from collate_bench import bursts, report  # noqa: E402
from splintr_amd import Tokenizer, _ffi, corpus  # noqa: E402
from splintr_amd.chat import ChatTemplate  # noqa: E402
from splintr_amd.device import DeviceBatch, chat_csr_device, encode_device, seqpack_rows_device  # noqa: E402

PAD_ID, IGNORE, K = 0, -100, 4
ROLES = ("user", "assistant", "user", "assistant")


def torch_next_fit(rows, labels, lengths, L, max_rows):
    """(input_ids, labels, position_ids) of seqpack_rows_device(..., strategy="next_fit", mask_first=True): the lengths go to the host, the
    placement is the reference's loop, the plan comes back, the rest is index arithmetic on the device"""
    dev, L_in = rows.device, rows.shape[1]
    lens = lengths.tolist()                              # (the synchronisation)
    row, col, r, f = [], [], -1, 0
    for l in lens:
        l = min(l, L)
        if l and (r < 0 or f + l > L):
            r, f = r + 1, 0
        row.append(r)
        col.append(f)
        f += l
    ln = lengths.clamp(max=L).long()
    base = (torch.tensor(row, device=dev) * L + torch.tensor(col, device=dev))
    seq = torch.repeat_interleave(torch.arange(len(lens), device=dev), ln)
    start = torch.cumsum(ln, 0) - ln
    pos = torch.arange(int(seq.numel()), device=dev) - start[seq]
    src, dst = seq * L_in + pos, base[seq] + pos
    out_ids = torch.full((max_rows * L,), PAD_ID, dtype=rows.dtype, device=dev)
    out_lab = torch.full((max_rows * L,), IGNORE, dtype=rows.dtype, device=dev)
    out_pos = torch.zeros(max_rows * L, dtype=torch.int32, device=dev)
    out_ids[dst] = rows.reshape(-1)[src]
    out_lab[dst] = torch.where(pos == 0, torch.full_like(pos, IGNORE).to(rows.dtype), labels.reshape(-1)[src])
    out_pos[dst] = pos.int()
    return out_ids.view(max_rows, L), out_lab.view(max_rows, L), out_pos.view(max_rows, L)


def plain(emit, samples, inner, nbytes=None):
    for name, xs in samples.items():
        s = sorted(xs)
        med = s[len(s) // 2]
        bw = f"   {nbytes / (med * 1e-3) / 1e9:8.1f} GB/s of algorithmic bytes" if nbytes and "gather" in name else ""
        emit(f"  {name:<44} median {med * 1e3:9.2f} us   min {s[0] * 1e3:9.2f}  max {s[-1] * 1e3:9.2f}{bw}   [{len(s)} bursts x {inner[name]} calls]")
    return {name: sorted(xs)[len(xs) // 2] for name, xs in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--seconds", type=float, default=0.3, help="device time per contender and shape")
    args = ap.parse_args()
    if not torch.cuda.is_available() or _ffi.lib().spl_device_count() == 0:
        sys.exit("seqpack_bench: no GPU")
    dev = torch.device("cuda", 0)
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    emit(f"seqpack_bench: {torch.cuda.get_device_name(0)}; per call, device events around bursts of back-to-back calls on one stream")
    lib = _ffi.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    verdicts = []
    for label, vocab, texts, row_len in (("C2 corpus.c2(1000) cl100k_base", "cl100k_base", corpus.c2(1000), 2048),
                                         ("C3 corpus.c3(10000) o200k_base", "o200k_base", corpus.c3(10000), 8192)):
        tok = Tokenizer.from_pretrained(vocab)
        tpl = ChatTemplate.chatml(tok)
        b = DeviceBatch(texts, dev)
        encode_device(tok, b)
        torch.cuda.synchronize()
        n_convs = b.n_docs // K
        turn_role = torch.tensor([tpl.role_of(r) for r in ROLES] * n_convs, dtype=torch.uint8, device=dev)
        conv_off = torch.arange(n_convs + 1, dtype=torch.int64, device=dev) * K
        emit()
        emit(f"== {label}: {n_convs} conversations of {K} turns, chat_device rows [{n_convs}, {row_len}]")
        for dtype, isz, name in ((torch.int32, 4, "int32"), (torch.int64, 8, "int64")):
            chat = chat_csr_device(tok, b.ids, b.out_off, b.n_docs, None, turn_role, conv_off, row_len, template=tpl, pad_id=PAD_ID, dtype=dtype)
            tokens = int(chat.lengths.sum().item())
            for seq_len, strategy in ((row_len, "next_fit"), (row_len, "best_fit_decreasing"), (2 * row_len, "next_fit"),
                                      (2 * row_len, "best_fit_decreasing")):
                kw = dict(pad_id=PAD_ID, strategy=strategy, labels=chat.labels, loss_mask=chat.loss_mask, role_ids=chat.role_ids,
                          special_tokens_mask=chat.special_tokens_mask)
                call = lambda: seqpack_rows_device(tok, chat.input_ids, chat.lengths, seq_len, **kw)
                got = call()
                n = got.n.tolist()
                assert int(got.status.item()) == 0 and n[1] == tokens
                R = n_convs
                # the gather reads every placed id, label and three bytes, and writes every element of nine [R, L] arrays
                nbytes = tokens * (2 * isz + 3) + R * seq_len * (2 * isz + 3 + 1 + 4 + 4)
                o = _ffi.SplSeqpackOpts((_ffi.SPL_COLLATE_I64 if isz == 8 else 0) | _ffi.SPL_SEQPACK_MASK_FIRST,
                                        _ffi.SPL_SEQPACK_BEST_FIT_DECREASING if strategy != "next_fit" else 0, seq_len, PAD_ID, IGNORE, (0, 255, 1, 0))
                p = lambda t: None if t is None else t.data_ptr()
                si = _ffi.SplSeqpackIn(n_convs, row_len, p(chat.input_ids), p(chat.lengths), None, p(chat.labels),
                                       [p(chat.loss_mask), p(chat.role_ids), p(chat.special_tokens_mask), None])
                pre = [None if t is None else torch.zeros_like(t) for t in got]   # (the status word is the caller's to clear)
                so = _ffi.SplSeqpackOut(R, p(pre[0]), p(pre[1]), [p(pre[5]), p(pre[6]), p(pre[7]), None], p(pre[2]), p(pre[3]), p(pre[4]), p(pre[9]),
                                        p(pre[10]), p(pre[11]), p(pre[12]), p(pre[13]))
                so0 = _ffi.SplSeqpackOut(0, p(pre[0]), None, [None] * 4, None, None, None, p(pre[9]), None, None, p(pre[12]), p(pre[13]))
                work = torch.empty(int(lib.spl_seqpack_work_bytes(n_convs, R, 0)), dtype=torch.uint8, device=dev)
                runs = {
                    f"seqpack_rows_device {strategy}": call,
                    "spl_seqpack_device preallocated (plan + gather)": lambda: lib.spl_seqpack_device(tok.handle, ctypes.byref(si), ctypes.byref(o), ctypes.byref(so), work.data_ptr(), st),
                    "spl_seqpack_device max_rows = 0 (plan alone)": lambda: lib.spl_seqpack_device(tok.handle, ctypes.byref(si), ctypes.byref(o), ctypes.byref(so0), work.data_ptr(), st),
                }
                title = f"seqpack [{n_convs}, {row_len}] -> [{R}, {seq_len}] {name} {strategy}"
                emit(f"{title}: rows needed {n[0]} of {n_convs}; padding share {100 * (1 - tokens / (n_convs * row_len)):.1f} % before, "
                     f"{100 * (1 - tokens / (max(n[0], 1) * seq_len)):.1f} % after (counts); {n[3]} sequences cut; cu_seqlens entries {n[2]}")
                if strategy == "next_fit":
                    want = torch_next_fit(chat.input_ids, chat.labels, chat.lengths, seq_len, R)
                    assert torch.equal(got.input_ids, want[0]) and torch.equal(got.labels, want[1]) and torch.equal(got.position_ids, want[2]), \
                        "the torch composition differs"
                    runs["torch composition"] = lambda: torch_next_fit(chat.input_ids, chat.labels, chat.lengths, seq_len, R)
                samples, inner = bursts(runs, args.seconds)
                if strategy == "next_fit":
                    ours = f"seqpack_rows_device {strategy}"
                    ok = report(emit, "  (the composition: input_ids, labels, position_ids; seqpack: all fourteen outputs)", nbytes,
                                {k: samples[k] for k in (ours, "torch composition")}, inner, ours, "torch composition")
                    plain(emit, {k: v for k, v in samples.items() if k not in (ours, "torch composition")}, inner)
                    verdicts.append((n_convs, seq_len, name, ok))
                    med = {k: sorted(v)[len(v) // 2] for k, v in samples.items()}
                else:
                    emit(f"  algorithmic bytes {nbytes / 1e6:.2f} MB")
                    med = plain(emit, samples, inner)
                both, plan = med["spl_seqpack_device preallocated (plan + gather)"], med["spl_seqpack_device max_rows = 0 (plan alone)"]
                emit(f"  -> gather = (plan + gather) - plan = {(both - plan) * 1e3:.2f} us = {nbytes / max(both - plan, 1e-9) / 1e6:.1f} GB/s of algorithmic bytes; "
                     f"plan alone {plan * 1e3:.2f} us = {plan * 1e6 / n_convs:.1f} ns per sequence")
                lib.spl_seqpack_device(tok.handle, ctypes.byref(si), ctypes.byref(o), ctypes.byref(so), work.data_ptr(), st)
                k = int(n[2])
                for i, (g, w) in enumerate(zip(pre, got)):
                    assert g is None or (torch.equal(g[:k], w[:k]) if i == 11 else torch.equal(g, w))
        del tok, b
    emit()
    for n_convs, row_len, name, ok in verdicts:
        emit(f"[{n_convs}, {row_len}] {name} next_fit: seqpack_rows_device " + ("beats" if ok else "does NOT beat") +
             " the torch composition by more than the two spreads together")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
