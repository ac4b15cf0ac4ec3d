#!/usr/bin/env python3
"""Time the device-side stop strings against what a serving loop does without them (GPU only).

    python tools/stop_bench.py [--out profiles/stop_match.txt]

The method is DESIGN 4.13's: the contenders run in alternation in this one process, 21 bursts after 3 warm-up rounds; printed per
contender are the median over the bursts of the time per STEP of the batch and the spread (max - min).  The state is carried from step
to step inside a burst (a burst walks the first STEPS steps of every sequence; every burst starts from fresh sequences).

Input: cl100k_base ids of corpus.c2 texts, 8 stops of 2 to 16 bytes.  Shapes: B = 256 and B = 4096 with K = 1, and B = 256 with K = 8.

  (a) host search         what there was before: add_tokens (no stops) to host strings, then per sequence the search a serving loop does
                          (str.find of every stop over the new text and max_stop_len - 1 characters in front of it), and the finished
                          mask copied back to the device; wall time around the synchronised step
  (b) add_tokens(stop=)   DeviceStreamingDecoder(stop=...).add_tokens over the same step, its copies to the host included; wall time
  (c) step_device(stop=)  the two device calls back to back, no host copy at all: the finished mask never leaves the GPU; device events
  (d) step_device         the same without stops: (c) - (d) is what the stop strings cost

Then (c)'s match call alone in its two forms ("stop_one_max") over 16 .. 1024 sequences.

The bar: (b) against (a), the gain set against the two spreads together; the case for the feature is (c)."""
import argparse
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from collate_bench import bursts  # noqa: E402
from stream_bench import STEPS, ROUNDS, WARM, stat, step_rows, wall_bursts  # noqa: E402
from splintr_amd import Tokenizer, _ffi  # noqa: E402
from splintr_amd.device import stop_table  # noqa: E402

STOPS = ["\n\n", "###", "</s>", "STOP", "Human:", " the end", "<|eot_id|>", "### Instruction:"]
MAX_STOP = max(len(s) for s in STOPS)


def event_bursts(contenders):
    """{name: [ms per step, one per burst]}: every burst is STEPS steps between two device events, nothing copied to the host"""
    out = {name: [] for name in contenders}
    for r in range(WARM + ROUNDS):
        for name, (fresh, step) in contenders.items():
            fresh()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for k in range(STEPS):
                step(k)
            b.record()
            torch.cuda.synchronize()
            if r >= WARM:
                out[name].append(a.elapsed_time(b) / STEPS)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--seconds", type=float, default=0.2, help="device time per contender and size of the two-forms sweep")
    args = ap.parse_args()
    if not torch.cuda.is_available() or _ffi.lib().spl_device_count() == 0:
        sys.exit("stop_bench: no GPU")
    dev = torch.device("cuda", 0)
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    def line(name, xs, unit):
        med, spread, lo, hi = stat(xs)
        emit(f"  {name:<48} median {med * 1e3:9.2f} us   min {lo * 1e3:9.2f}  max {hi * 1e3:9.2f}  spread {spread * 1e3:8.2f} us   [{len(xs)} bursts x {unit}]")
        return med, spread

    L = _ffi.lib()
    tok = Tokenizer.from_pretrained("cl100k_base")
    st = torch.cuda.current_stream(dev).cuda_stream
    emit(f"stop_bench: {torch.cuda.get_device_name(0)}; library {os.path.basename(_ffi.LIB_PATH)}; cl100k_base, ids of corpus.c2 texts, "
         f"{len(STOPS)} stops of {min(map(len, STOPS))} to {MAX_STOP} bytes; per STEP of the batch")
    all_ok = True
    for B, K in ((256, 1), (4096, 1), (256, 8)):
        d_rows = torch.from_numpy(step_rows(tok, B, K)).to(dev)
        emit()
        emit(f"== B = {B}, K = {K}: {STEPS} steps a burst, state carried across the steps")
        plain = tok.device_streaming_decoder(B)
        dec = tok.device_streaming_decoder(B, stop=STOPS)
        text, done = [], []

        def host_fresh():
            plain.reset()
            text[:] = [""] * B
            done[:] = [False] * B

        def host_step(k):
            pieces = plain.add_tokens(d_rows[k])
            for b, p in enumerate(pieces):
                if p is None or done[b]:
                    continue
                t = text[b] + p
                lo = max(0, len(text[b]) - MAX_STOP + 1)
                for s in STOPS:
                    if t.find(s, lo) >= 0:
                        done[b] = True
                        break
                text[b] = t
            return torch.tensor(done, dtype=torch.bool).to(dev)         # the finished mask the sampler needs, back on the device

        def dev_step(k):
            return dec.add_tokens(d_rows[k])
        # the two agree on who has finished, step for step
        host_fresh()
        dec.reset()
        for k in range(STEPS):
            m = host_step(k)
            dev_step(k)
            assert torch.equal(m, dec.finished), (B, K, k)
        w = wall_bursts({"a": (host_fresh, host_step), "b": (dec.reset, dev_step)})
        ma, sa = line("(a) add_tokens + host search + mask H2D (wall)", w["a"], f"{STEPS} steps")
        mb, sb = line("(b) add_tokens(stop=...) (wall)", w["b"], f"{STEPS} steps")
        ok = ma - mb > sa + sb
        all_ok &= ok
        emit(f"  -> (b) is {ma / mb:.2f}x (a); gain {(ma - mb) * 1e3:.1f} us against the two spreads together {(sa + sb) * 1e3:.1f} us: {'PASS' if ok else 'MISS'}")
        e = event_bursts({"c": (dec.reset, lambda k: dec.step_device(d_rows[k])), "d": (plain.reset, lambda k: plain.step_device(d_rows[k]))})
        mc, sc = line("(c) step_device(stop=...) (device events)", e["c"], f"{STEPS} steps")
        md, sd = line("(d) step_device without stops (device events)", e["d"], f"{STEPS} steps")
        emit(f"  -> the stop strings cost (c) - (d) = {(mc - md) * 1e3:.2f} us a step; the finished mask stays on the device")
        del dec, plain

    emit()
    emit("== the match call alone, K = 1: one launch against three launches, device events (the option \"stop_one_max\" picks the form)")
    table = stop_table(STOPS, dev)
    cross = None
    for B in (16, 32, 48, 64, 80, 96, 128, 192, 256, 512, 1024):
        d_rows = torch.from_numpy(step_rows(tok, B, 1)).to(dev)
        dec = tok.device_streaming_decoder(B, stop=STOPS)
        for k in range(4):                                              # a state in mid-stream, and step 4's bytes as the input
            dec.step_device(d_rows[k])
        state = dec.stop_state.clone()
        plain = tok.device_streaming_decoder(B)
        for k in range(4):
            plain.step_device(d_rows[k])
        inb, in_off = plain.step_device(d_rows[4])
        s_out = torch.empty_like(state)
        out = torch.empty(inb.numel() + 64 * B, dtype=torch.uint8, device=dev)
        off = torch.empty(B + 1, dtype=torch.int64, device=dev)
        hit = torch.empty(B, dtype=torch.int32, device=dev)

        def call(limit):
            def f():
                L.spl_set_option(tok.handle, b"stop_one_max", limit)
                return L.spl_stop_match_device(tok.handle, inb.data_ptr(), inb.numel(), in_off.data_ptr(), B, table.data_ptr(), None, None, 0,
                                               state.data_ptr(), s_out.data_ptr(), out.data_ptr(), out.numel(), off.data_ptr(), hit.data_ptr(), st)
            return f
        samples, inner = bursts({"one": call(1024), "three": call(0)}, args.seconds)
        (m1, s1, _, _), (m3, s3, _, _) = stat(samples["one"]), stat(samples["three"])
        emit(f"  B = {B:5d}   one launch {m1 * 1e3:8.2f} us (spread {s1 * 1e3:6.2f})   three launches {m3 * 1e3:8.2f} us (spread {s3 * 1e3:6.2f})   "
             f"{'one' if m1 < m3 else 'three'} is faster")
        if cross is None and m1 >= m3:
            cross = B
        del dec, plain
    emit(f"  the medians cross {'at or below B = %d' % cross if cross else 'beyond B = 1024: the one-launch form is faster at every size it can take'}")
    emit()
    emit("(b) faster than (a) at every shape by more than the two spreads together: " + ("yes" if all_ok else "NO"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
