"""N-gram drafting on the GPU against what it replaces and against the bandwidth floor -> profiles/ngram_draft.txt.

  (n) the call          spl_ngram_draft_device, one new id per sequence appended and one draft of 8 ids (one branch) or 4 x 8 (four) searched,
                        with slices = 1, 2, 4, 8, 16, 32 and with the automatic choice (0); the chosen number is printed
  (c) the floor         a device-to-device copy of the same history bytes (torch's copy_), in the same run: the search reads every id once
  (h) what it replaces  the step's ids to the host (D2H, [B] ids), a numpy suffix search per sequence over the host's copy of the history
                        (vLLM's ngram proposer: the last n ids, n = max_n .. min_n, against every window), the draft back (H2D, [B, 8]).
                        Wall time; searched for at most HOST_SEQS sequences and scaled to B, which the line says

B = 4, 32, 256, 4 096; histories of 1 K, 8 K and 64 K ids (capacity = length + 64), int32, ids uniform over 32 000 with the last 4 ids
planted once at two thirds of the history, so that one candidate survives the first compare in about 32 000 and the call is what a
sparse history costs: its traffic.  Device events around bursts of CALLS calls; the lengths are reset between bursts, outside the
events.  No number here is a bar: none existed.  The crossover of the automatic choice (ngram_auto_slices, spl_ngram_host.h) is set
from the table this prints."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from stream_bench import stat  # noqa: E402
from splintr_amd import Tokenizer, _ffi  # noqa: E402
from splintr_amd import device as dv  # noqa: E402

CALLS, WARM, ROUNDS, HOST_SEQS, VOCAB = 16, 2, 9, 32, 32000
SLICES = (1, 2, 4, 8, 16, 32, 0)


def host_search(h, min_n, max_n, depth):
    """the latest earlier occurrence of the longest suffix n-gram, by numpy windows -> the draft"""
    for n in range(max_n, min_n - 1, -1):
        if len(h) <= n:
            continue
        w = np.lib.stride_tricks.sliding_window_view(h[:-1], n)
        hit = np.flatnonzero((w == h[-n:]).all(1))
        if hit.size:
            e = int(hit[-1]) + n
            return h[e:e + depth]
    return h[:0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--sizes", default="4,32,256,4096")
    ap.add_argument("--lengths", default="1024,8192,65536")
    args = ap.parse_args()
    if not torch.cuda.is_available() or _ffi.lib().spl_device_count() == 0:
        sys.exit("ngram_bench: no GPU")
    dev = torch.device("cuda", 0)
    tok = Tokenizer.from_pretrained("cl100k_base")
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    emit(f"ngram_bench: {torch.cuda.get_device_name(0)}; library {os.path.basename(_ffi.LIB_PATH)}; bursts of {CALLS} calls, {ROUNDS} bursts; us per CALL, median (spread)")
    opts = dict(min_n=2, max_n=4, depth=8)
    for B in map(int, args.sizes.split(",")):
        dv.ngram_reserve(tok, B)
        for L in map(int, args.lengths.split(",")):
            cap = L + 64
            g = torch.Generator(device=dev).manual_seed(B + L)
            hist = torch.randint(0, VOCAB, (B, cap), dtype=torch.int32, device=dev, generator=g)
            at = 2 * L // 3
            hist[:, at:at + 4] = hist[:, L - 4:L]
            keep, other = hist.clone(), torch.empty_like(hist)
            length = torch.full((B,), L, dtype=torch.int32, device=dev)
            new = torch.randint(0, VOCAB, (B, 1), dtype=torch.int32, device=dev, generator=g)
            one = torch.ones(B, dtype=torch.int32, device=dev)
            emit()
            emit(f"== B = {B}, history {L} ids ({B * L * 4 / 1e6:.1f} MB)")
            res = {}
            for branches in (1, 4):
                outs = dv.ngram_draft_device(tok, hist, length, branches=branches, **opts)             # (nothing appended: the history still ends with the planted ids)
                assert (outs.from_[:, 0] == at + 4).all().item() and (outs.match[:, 0] == 4).all().item(), "the planted repeat was not found"
                contenders = {f"n{branches}/{s}": (lambda s=s, branches=branches, outs=outs: dv.ngram_draft_device(
                    tok, hist, length, new=new, new_len=one, branches=branches, slices=s, out=outs, **opts)) for s in SLICES}
                if branches == 1:
                    contenders["copy"] = lambda: other.copy_(hist)
                t = {k: [] for k in contenders}
                for r in range(WARM + ROUNDS):
                    for k, call in contenders.items():
                        length.fill_(L)
                        hist[:, L:].copy_(keep[:, L:])
                        torch.cuda.synchronize()
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        for _ in range(CALLS):
                            call()
                        b.record()
                        torch.cuda.synchronize()
                        if r >= WARM:
                            t[k].append(a.elapsed_time(b) * 1e3 / CALLS)
                res.update({k: stat(v) for k, v in t.items()})
            length.fill_(L)
            # what the call replaces, wall: D2H of the step's ids, the search on the host's history, H2D of the draft
            n_host = min(B, HOST_SEQS)
            h_hist = hist.cpu().numpy()[:, :L + 1].copy()
            pin_in, pin_out = torch.empty((B, 1), dtype=torch.int32).pin_memory(), torch.zeros((B, 8), dtype=torch.int32).pin_memory()
            d_draft = torch.empty((B, 8), dtype=torch.int32, device=dev)
            walls = []
            for r in range(3):
                t0 = time.perf_counter()
                pin_in.copy_(new, non_blocking=True)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for b in range(n_host):
                    h_hist[b, L] = pin_in[b, 0]
                    d = host_search(h_hist[b], opts["min_n"], opts["max_n"], opts["depth"])
                    pin_out[b, :len(d)] = torch.from_numpy(d)
                t2 = time.perf_counter()
                d_draft.copy_(pin_out, non_blocking=True)
                torch.cuda.synchronize()
                t3 = time.perf_counter()
                walls.append(((t1 - t0) + (t3 - t2) + (t2 - t1) * B / n_host) * 1e6)
            for branches in (1, 4):
                row = "  ".join(f"S={s or 'auto'} {res[f'n{branches}/{s}'][0]:9.1f} ({res[f'n{branches}/{s}'][1]:6.1f})" for s in SLICES)
                emit(f"  (n) branches {branches}: {row}")
            best = min(SLICES[:-1], key=lambda s: res[f"n1/{s}"][0])
            emit(f"  (c) copy of the history: {res['copy'][0]:9.1f} ({res['copy'][1]:6.1f})   (n, one branch, S=1) / (c) = {res['n1/1'][0] / res['copy'][0]:5.2f}   "
                 f"best forced S = {best}; auto / best = {res['n1/0'][0] / res[f'n1/{best}'][0]:5.2f}")
            emit(f"  (h) host route, wall, searched for {n_host} of {B} sequences and scaled: {stat(walls)[0]:12.1f} us   (h) / (n, auto) = {stat(walls)[0] / res['n1/0'][0]:8.1f}x")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
