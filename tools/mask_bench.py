"""The bitmask-to-logits kernel and the UTF-8 continuation masks on the GPU -> profiles/mask_apply.txt.

cl100k_base and o200k_base, B = 256 and 4096 rows of logits, bf16 and f32 (rows padded to a multiple of 16 bytes, so a lane's piece is a
byte -- f32: a nibble -- of the mask and the bytes moved can be counted from the mask itself); bursts of STEPS calls between two device
events, as tools/heal_bench.py times its device calls.

  (a) spl_mask_apply_device on three mask populations: the healer's begin-state masks (corpus.c2 prompts cut inside a word, begin auto,
      max_back 3; the rows of free sequences hold ones), UTF-8 start-class rows (every sequence fresh), all rows free with `live`
  (b) the torch-op composition TokenHealer.apply was made of before -- the mask expanded to one int32 per bit, then masked_fill_ -- on the
      same tensors
  (c) spl_utf8_mask_device alone, and with and_into, over fresh sequences and over a mix of the eight classes

(a) counts as faster than (b) only where the gain exceeds the two spreads together.  For (a) the bytes the three lane cases move (nothing;
a 16-byte store; a 16-byte load and store), the mask words and the live bytes are counted and set against the 6.29 TB/s a float4 copy
reaches on this GPU (the guide's measured figure; the model is arithmetic, the times are measured)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from heal_bench import cut_prompts  # noqa: E402
from stop_bench import event_bursts  # noqa: E402
from stream_bench import STEPS, stat  # noqa: E402
from splintr_amd import Tokenizer, _ffi  # noqa: E402
from splintr_amd import device as dv  # noqa: E402

COPY_RATE = 6.29e12        # bytes per second: the measured float4 copy rate of an MI355X


def former_apply(logits, mask, n_words):
    """what TokenHealer.apply did before the kernel"""
    V = min(int(logits.shape[1]), 32 * n_words)
    bits = ((mask.unsqueeze(-1) >> torch.arange(32, device=mask.device, dtype=torch.int32)) & 1).reshape(mask.shape[0], -1)
    logits[:, :V].masked_fill_(bits[:, :V] == 0, float("-inf"))
    return logits


def traffic(mask, live, V, es):
    """bytes the kernel moves for these masks over rows that begin on a 16-byte boundary: (stored without a load, loaded and stored, mask
    words read, live bytes read, pieces that did nothing)"""
    B, nw = mask.shape
    rows = torch.ones(B, dtype=torch.bool, device=mask.device) if live is None else live != 0
    by = mask.view(torch.uint8).reshape(B, -1)                                 # a byte: eight columns
    if es == 4:                                                                # a nibble: four columns
        by = torch.stack((by & 15, by >> 4), -1).reshape(B, -1)
        full = 15
    else:
        full = 255
    per = 16 // es
    n_whole = V // per                                                         # (the tail piece stores elements: not counted)
    by = by[:, :n_whole][rows]
    zero, ones = int((by == 0).sum().item()), int((by == full).sum().item())
    mixed = by.numel() - zero - ones
    n_live = int(rows.sum().item())
    return zero * 16, mixed * 32, n_live * ((V + 31) // 32) * 4, (0 if live is None else B), ones


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--vocabs", default="cl100k_base,o200k_base")
    ap.add_argument("--sizes", default="256,4096")
    args = ap.parse_args()
    if not torch.cuda.is_available() or _ffi.lib().spl_device_count() == 0:
        sys.exit("mask_bench: no GPU")
    dev = torch.device("cuda", 0)
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    def line(name, xs):
        med, spread, lo, hi = stat(xs)
        emit(f"  {name:<56} median {med * 1e3:9.2f} us   min {lo * 1e3:9.2f}  max {hi * 1e3:9.2f}  spread {spread * 1e3:8.2f} us   [{len(xs)} bursts]")
        return med, spread

    emit(f"mask_bench: {torch.cuda.get_device_name(0)}; library {os.path.basename(_ffi.LIB_PATH)}; bursts of {STEPS} calls between two device "
         f"events; per CALL; {torch.cuda.mem_get_info(0)[1] / 2**30:.0f} GiB of HBM, so B = 4096's 1.6 GB temporary of (b) fits")
    all_ok = True
    for name in args.vocabs.split(","):
        tok = Tokenizer.from_pretrained(name)
        V, nw = tok.vocab_size, dv.heal_n_words(tok)
        dv.utf8_mask_reserve(tok)
        for B in map(int, args.sizes.split(",")):
            enc = tok.encode_batch(cut_prompts(B))
            K = max(len(e) for e in enc)
            rows = torch.zeros((B, K), dtype=torch.int64)
            for b, e in enumerate(enc):
                rows[b, :len(e)] = torch.tensor(e, dtype=torch.int64)
            healer = dv.TokenHealer(tok, B, max_back=3, auto=True)
            healer.begin(rows.to(dev), torch.tensor([len(e) for e in enc], dtype=torch.int32, device=dev))
            fresh = torch.zeros(B, dtype=torch.int64, device=dev)
            start_mask, _ = dv.utf8_mask_device(tok, fresh)
            ones = torch.full((B, nw), -1, dtype=torch.int32, device=dev)
            pops = [("healer's begin-state masks", healer.mask, None), ("healer's masks, live rows only", healer.mask, healer.live),
                    ("UTF-8 start-class rows", start_mask, None), ("all rows free, live 0", ones, torch.zeros(B, dtype=torch.uint8, device=dev))]
            emit()
            emit(f"== {name}, B = {B}: V = {V}, n_words = {nw}; {int(healer.n[0].item())} of {B} sequences constrained at begin")
            for dtype, es in ((torch.bfloat16, 2), (torch.float32, 4)):
                Vp = (V + 16 // es - 1) // (16 // es) * (16 // es)
                logits = torch.randn((B, Vp), device=dev, dtype=torch.float32).to(dtype)[:, :V]
                emit(f"  -- {str(dtype).split('.')[1]}: {B * V * es / 1e6:.0f} MB of logits")
                for what, mask, live in pops:
                    e = event_bursts({"a": (lambda: None, lambda k: dv.mask_apply_device(tok, logits, mask, live=live))})
                    ma, sa = line(f"(a) spl_mask_apply_device, {what}", e["a"])
                    st, ls, mw, lv, idle = traffic(mask, live, V, es)
                    moved = st + ls + mw + lv
                    emit(f"      moved: {st / 1e6:.1f} MB stored without a load, {ls / 1e6:.1f} MB loaded and stored, {mw / 1e6:.1f} MB of mask, {lv} live bytes; "
                         f"{idle} pieces untouched -> {moved / (ma * 1e-3) / 1e12:.2f} TB/s, {100 * moved / (ma * 1e-3) / COPY_RATE:.0f} % of the {COPY_RATE / 1e12:.2f} TB/s copy rate")
                    if live is None:
                        e = event_bursts({"b": (lambda: None, lambda k: former_apply(logits, mask, nw))})
                        mb, sb = line("(b) the torch-op composition on the same tensors", e["b"])
                        ok = mb - ma > sa + sb
                        all_ok &= ok
                        emit(f"  -> (a) is {mb / ma:.1f}x (b); gain {(mb - ma) * 1e3:.1f} us against the two spreads together {(sa + sb) * 1e3:.1f} us: {'PASS' if ok else 'MISS'}")
                del logits
            mixed = torch.tensor([[0, 0xC3 | 1 << 24, 0xE1 | 1 << 24, 0xF1 | 1 << 24, 0xE0 | 1 << 24, 0xED | 1 << 24, 0xF0 | 1 << 24, 0xF4 | 1 << 24][b % 8]
                                  for b in range(B)], dtype=torch.int64, device=dev)
            out = torch.empty((B, nw), dtype=torch.int32, device=dev)
            for what, state in (("fresh sequences", fresh), ("a mix of the eight classes", mixed)):
                e = event_bursts({"c": (lambda: None, lambda k: dv.utf8_mask_device(tok, state, out=out)),
                                  "d": (lambda: None, lambda k: dv.utf8_mask_device(tok, state, out=healer.mask, and_into=True))})
                mc, _ = line(f"(c) spl_utf8_mask_device, {what}", e["c"])
                md, _ = line(f"(c) ... with and_into (into the healer's mask)", e["d"])
                nbytes = B * nw * 4
                emit(f"      {nbytes / 1e6:.1f} MB of mask: written at {nbytes / (mc * 1e-3) / 1e12:.2f} TB/s; read and written at {2 * nbytes / (md * 1e-3) / 1e12:.2f} TB/s")
    emit()
    emit(f"(a) faster than (b) at every shape and population by more than the two spreads together: {'yes' if all_ok else 'NO'}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
