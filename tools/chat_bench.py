#!/usr/bin/env python3
"""Time spl_chat_device against the torch-op composition a user would otherwise write (GPU only).

Method as tools/collate_bench.py (its bursts / report are used): the contenders produce IDENTICAL input_ids, labels and attention_mask
(asserted once, before any timing) from the same device-resident encode result and are timed in alternation in this one process -- a
sample is a burst of back-to-back calls between two device events on the current stream, the median over the bursts is reported with its
spread.

    python tools/chat_bench.py [--out profiles/chat.txt]

Cases, ChatML on the vocabulary's own control tokens, turns user / assistant / user / assistant, labels on the assistant's content and
footer, the body cut on the right, padding on the right, with the generation prompt:
  C2   corpus.c2(1000) as 250 conversations of 4 turns, rows [250, 2048], int32 and int64
  C3   corpus.c3(10000) as 2500 conversations of 4 turns, rows [2500, 8192], int32 and int64
Lines per case: chat_device (allocates its ten outputs per call; the composition allocates its three), the torch composition (written
for a FIXED number of turns per conversation with the role a function of the turn's position -- the general ragged case needs a
segmented scan on top), spl_chat_device alone (the C-ABI call into preallocated outputs: the two launches)."""
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
from splintr_amd.device import DeviceBatch, chat_csr_device, encode_device  # noqa: E402

PAD_ID, IGNORE, K = 0, -100, 4
ROLES = ("user", "assistant", "user", "assistant")


def torch_chat(ids, off, n_convs, tpl, L, dtype):
    """(input_ids, labels, attention_mask) of chat_csr_device(..., add_generation_prompt=True) for conversations of K turns each, turn k of
    conversation c being document c * K + k with the role ROLES[k]: per turn three masked selects over the [n_convs, L] grid"""
    dev = ids.device
    n_bos, gen = len(tpl.bos), torch.tensor(tpl.generation, dtype=torch.int64, device=dev)
    end = L - len(tpl.generation)                      # body columns are [n_bos, end)
    col = torch.arange(L, device=dev).unsqueeze(0)
    rows = torch.full((n_convs, L), PAD_ID, dtype=torch.int64, device=dev)
    labels = torch.full((n_convs, L), IGNORE, dtype=torch.int64, device=dev)
    for j, v in enumerate(tpl.bos):
        rows[:, j] = v
    pos = torch.full((n_convs, 1), n_bos, dtype=torch.int64, device=dev)
    docs = torch.arange(n_convs, device=dev) * K
    body = col < end
    for k, role in enumerate(ROLES):
        h, f = (torch.tensor(x, dtype=torch.int64, device=dev) for x in tpl.roles[role])
        o0 = off[docs + k].unsqueeze(1)
        ln = off[docs + k + 1].unsqueeze(1) - o0
        trained = role in tpl.train
        for kind, n_seg in (("header", h.numel()), ("content", ln), ("footer", f.numel())):
            seg = (col >= pos) & (col < pos + n_seg) & body
            j = col - pos
            if kind == "header":
                val = h[j.clamp(0, h.numel() - 1)]
            elif kind == "footer":
                val = f[j.clamp(0, f.numel() - 1)]
            else:
                val = ids[(o0 + j).clamp_(0, ids.numel() - 1)].long()
            rows = torch.where(seg, val, rows)
            if trained and kind != "header":
                labels = torch.where(seg, val, labels)
            pos = pos + n_seg
    used = pos.clamp(max=end)
    g = col - used
    seg = (g >= 0) & (g < gen.numel())
    rows = torch.where(seg, gen[g.clamp(0, gen.numel() - 1)], rows)
    return rows.to(dtype), labels.to(dtype), (col < used + gen.numel()).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--seconds", type=float, default=0.4, help="device time per contender and shape")
    args = ap.parse_args()
    if not torch.cuda.is_available() or _ffi.lib().spl_device_count() == 0:
        sys.exit("chat_bench: no GPU")
    dev = torch.device("cuda", 0)
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    emit(f"chat_bench: {torch.cuda.get_device_name(0)}; per call, device events around bursts of back-to-back calls on one stream")
    L = _ffi.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    verdicts = []
    for label, vocab, texts, row_len in (("C2 corpus.c2(1000) cl100k_base", "cl100k_base", corpus.c2(1000), 2048),
                                         ("C3 corpus.c3(10000) o200k_base", "o200k_base", corpus.c3(10000), 8192)):
        tok = Tokenizer.from_pretrained(vocab)
        tpl = ChatTemplate.chatml(tok)
        b = DeviceBatch(texts, dev)
        encode_device(tok, b)
        torch.cuda.synchronize()
        n_docs = b.n_docs
        n_convs, n_turns = n_docs // K, n_docs
        turn_role = torch.tensor([tpl.role_of(r) for r in ROLES] * n_convs, dtype=torch.uint8, device=dev)
        conv_off = torch.arange(n_convs + 1, dtype=torch.int64, device=dev) * K
        ids, off = b.ids, b.out_off
        emit()
        emit(f"== {label}: {n_docs} documents, {int(off[-1].item())} tokens; {n_convs} conversations of {K} turns")
        for dtype, isz, name in ((torch.int32, 4, "int32"), (torch.int64, 8, "int64")):
            kw = dict(template=tpl, pad_id=PAD_ID, add_generation_prompt=True, dtype=dtype)
            call = lambda: chat_csr_device(tok, ids, off, n_docs, None, turn_role, conv_off, row_len, **kw)
            got = call()
            want = torch_chat(ids, off, n_convs, tpl, row_len, dtype)
            assert torch.equal(got.input_ids, want[0]) and torch.equal(got.labels, want[1]) and torch.equal(got.attention_mask, want[2]), \
                "the torch composition differs"
            assert int(got.status.item()) == 0
            tc = got.turn_cols.long()
            kept_ids = int((tc[:, 1] - tc[:, 0]).clamp(min=0).sum().item())
            cut = int((got.kept[:, 1] > 0).sum().item())
            nbytes = 4 * kept_ids + 25 * n_turns + n_convs * row_len * (2 * isz + 4) + 44 * n_convs
            o = _ffi.SplChatOpts((_ffi.SPL_COLLATE_I64 if isz == 8 else 0), row_len, PAD_ID, IGNORE, list(tpl.roles.values()),
                                 tpl.train_content_mask, tpl.train_footer_mask, tpl.bos, tpl.generation)
            pre = [torch.empty_like(t) for t in got[:9]] + [torch.zeros_like(got.status)]
            work = torch.empty(int(L.spl_chat_work_bytes(n_turns, n_convs)), dtype=torch.uint8, device=dev)
            p = [t.data_ptr() for t in pre]
            runs = {
                "spl chat_device": call,
                "torch composition": lambda: torch_chat(ids, off, n_convs, tpl, row_len, dtype),
                "spl_chat_device preallocated": lambda: L.spl_chat_device(
                    tok.handle, ids.data_ptr(), off.data_ptr(), n_docs, None, turn_role.data_ptr(), None, n_turns, conv_off.data_ptr(), n_convs,
                    ctypes.byref(o), p[0], p[1], p[4], p[2], p[3], p[5], p[6], p[7], p[8], p[9], work.data_ptr(), st),
            }
            samples, inner = bursts(runs, args.seconds)
            ok = report(emit, f"chat [{n_convs}, {row_len}] {name}: ten outputs (the composition: input_ids, labels, attention_mask); {cut} rows cut", nbytes,
                        samples, inner, "spl chat_device", "torch composition")
            verdicts.append((n_convs, row_len, name, ok))
            assert all(torch.equal(g, w) for g, w in zip(pre, got))
        del tok, b
    emit()
    for n_convs, row_len, name, ok in verdicts:
        emit(f"[{n_convs}, {row_len}] {name}: chat_device " + ("beats" if ok else "does NOT beat") + " the torch composition by more than the spread")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
