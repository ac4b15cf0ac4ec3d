#!/usr/bin/env python3
"""Time the device-side batched streaming decode against what a serving loop does without it (GPU only).

    python tools/stream_bench.py [--out profiles/stream_decode.txt]

The method is DESIGN 4.10's: the contenders run in alternation in this one process, 21 bursts after 3 warm-up rounds; printed per
contender are the median over the bursts of the time per call (a call is one STEP of the batch) and the spread (max - min).

Shapes, all real encodes of corpus.c2 texts by cl100k_base, the state carried from step to step inside a burst (a burst walks the first
STEPS steps of every sequence; every burst starts from fresh decoders):  B = 256 and B = 4096 with K = 1, and B = 256 with K = 8.

  (a) host loop           what there was before: the step's ids to the host (D2H), then B host add_token / add_tokens calls;
                          wall time (time.perf_counter) around the synchronised step
  (b) add_tokens          DeviceStreamingDecoder.add_tokens over the same step, its copies to the host included; wall time likewise
  (c) device call alone   spl_stream_decode_device into preallocated outputs, device events around the burst; the one-launch and the
                          three-launch form ("stream_one_max") at batch sizes on both sides of the threshold
  (d) decode_rows_device  the same rows through the bulk decode: a floor that does no UTF-8 work -- context, not a bar

The bar: (b) faster than (a) at every shape by more than the two spreads together."""
import argparse
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from collate_bench import bursts  # noqa: E402
from splintr_amd import Tokenizer, _ffi, corpus  # noqa: E402
from splintr_amd.device import decode_rows_device, decode_reserve  # noqa: E402

ROUNDS, WARM, STEPS = 21, 3, 16


def step_rows(tok, B, K):
    """[STEPS, B, K] ids: the first STEPS * K tokens of B c2 documents (a shorter document repeats)"""
    ids = tok.encode_batch(corpus.c2(B))
    rows = np.zeros((B, STEPS * K), dtype=np.int64)
    for b, x in enumerate(ids):
        x = (x * (STEPS * K // max(len(x), 1) + 1))[:STEPS * K] if x else [0] * (STEPS * K)
        rows[b] = x
    return np.ascontiguousarray(rows.reshape(B, STEPS, K).transpose(1, 0, 2))


def wall_bursts(contenders):
    """{name: [ms per step, one per burst]}: every burst is STEPS synchronised steps, timed on the host"""
    out = {name: [] for name in contenders}
    for r in range(WARM + ROUNDS):
        for name, (fresh, step) in contenders.items():
            fresh()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(STEPS):
                step(k)
            torch.cuda.synchronize()
            if r >= WARM:
                out[name].append((time.perf_counter() - t0) * 1e3 / STEPS)
    return out


def stat(xs):
    s = sorted(xs)
    return s[len(s) // 2], s[-1] - s[0], s[0], s[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--seconds", type=float, default=0.2, help="device time per contender and shape of (c) and (d)")
    args = ap.parse_args()
    if not torch.cuda.is_available() or _ffi.lib().spl_device_count() == 0:
        sys.exit("stream_bench: no GPU")
    dev = torch.device("cuda", 0)
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    def line(name, xs, unit_calls):
        med, spread, lo, hi = stat(xs)
        emit(f"  {name:<44} median {med * 1e3:9.2f} us   min {lo * 1e3:9.2f}  max {hi * 1e3:9.2f}  spread {spread * 1e3:8.2f} us   [{len(xs)} bursts x {unit_calls}]")
        return med, spread

    L = _ffi.lib()
    tok = Tokenizer.from_pretrained("cl100k_base")
    st = torch.cuda.current_stream(dev).cuda_stream
    emit(f"stream_bench: {torch.cuda.get_device_name(0)}; library {os.path.basename(_ffi.LIB_PATH)}; cl100k_base, ids of corpus.c2 texts; per STEP of the batch")
    all_ok = True
    for B, K in ((256, 1), (4096, 1), (256, 8)):
        rows = step_rows(tok, B, K)
        d_rows = torch.from_numpy(rows).to(dev)
        decode_reserve(tok, B * K)
        emit()
        emit(f"== B = {B}, K = {K}: {STEPS} steps a burst, state carried across the steps")
        host = []
        dec = tok.device_streaming_decoder(B)

        def host_fresh():
            host[:] = [tok.streaming_decoder() for _ in range(B)]

        def host_step(k):
            step = d_rows[k].cpu().tolist()                           # the D2H of the step's ids (synchronises)
            if K == 1:
                return [h.add_token(r[0]) for h, r in zip(host, step)]
            return [h.add_tokens(r) for h, r in zip(host, step)]

        def dev_step(k):
            return dec.add_tokens(d_rows[k])
        # the two produce the same text, step for step
        host_fresh()
        dec.reset()
        for k in range(STEPS):
            assert host_step(k) == dev_step(k), (B, K, k)
        w = wall_bursts({"a": (host_fresh, host_step), "b": (dec.reset, dev_step)})
        ma, sa = line("(a) D2H + B host add_token calls (wall)", w["a"], f"{STEPS} steps")
        mb, sb = line("(b) DeviceStreamingDecoder.add_tokens (wall)", w["b"], f"{STEPS} steps")
        ok = ma - mb > sa + sb
        all_ok &= ok
        emit(f"  -> (b) is {ma / mb:.1f}x (a); gain {(ma - mb) * 1e3:.1f} us against the two spreads together {(sa + sb) * 1e3:.1f} us: {'PASS' if ok else 'MISS'}")
        # (c) the device call alone, (d) the bulk decode on the same rows
        state = torch.zeros(B, dtype=torch.int64, device=dev)
        s_out = torch.empty_like(state)
        out = torch.empty(16 * B * K + 16, dtype=torch.uint8, device=dev)
        off = torch.empty(B + 1, dtype=torch.int64, device=dev)
        o = _ffi.SplDecodeOpts(_ffi.SPL_DECODE_I64, K)
        row0 = d_rows[1]
        runs = {"(c) spl_stream_decode_device alone": lambda: L.spl_stream_decode_device(
                    tok.handle, row0.data_ptr(), None, B, ctypes.byref(o), 0, None, state.data_ptr(), s_out.data_ptr(), out.data_ptr(), out.numel(),
                    off.data_ptr(), st),
                "(d) decode_rows_device (no UTF-8 work)": lambda: decode_rows_device(tok, row0, None, max_bytes=16 * B * K)}
        samples, inner = bursts(runs, args.seconds)
        for name, xs in samples.items():
            line(name, xs, f"{inner[name]} calls")
        del dec

    # the two launch shapes on both sides of the threshold
    emit()
    emit("== (c) one launch against three launches, K = 1, device events (the option \"stream_one_max\" picks the form)")
    cross = None
    for B in (16, 32, 48, 64, 80, 96, 128, 256, 1024):
        rows = torch.from_numpy(step_rows(tok, B, 1)[1]).to(dev)
        state = torch.zeros(B, dtype=torch.int64, device=dev)
        s_out = torch.empty_like(state)
        out = torch.empty(16 * B + 16, dtype=torch.uint8, device=dev)
        off = torch.empty(B + 1, dtype=torch.int64, device=dev)
        o = _ffi.SplDecodeOpts(_ffi.SPL_DECODE_I64, 1)

        def call(limit):
            def f():
                L.spl_set_option(tok.handle, b"stream_one_max", limit)
                return L.spl_stream_decode_device(tok.handle, rows.data_ptr(), None, B, ctypes.byref(o), 0, None, state.data_ptr(), s_out.data_ptr(),
                                                  out.data_ptr(), out.numel(), off.data_ptr(), st)
            return f
        samples, inner = bursts({"one": call(1024), "three": call(0)}, args.seconds)
        (m1, s1, _, _), (m3, s3, _, _) = stat(samples["one"]), stat(samples["three"])
        emit(f"  B = {B:5d}   one launch {m1 * 1e3:8.2f} us (spread {s1 * 1e3:6.2f})   three launches {m3 * 1e3:8.2f} us (spread {s3 * 1e3:6.2f})   "
             f"{'one' if m1 < m3 else 'three'} is faster")
        if cross is None and m1 >= m3:
            cross = B
    emit(f"  the medians cross {'at or below B = %d' % cross if cross else 'beyond B = 1024: the one-launch form is faster at every size it can take'}")
    emit()
    emit("(b) faster than (a) at every shape by more than the two spreads together: " + ("yes" if all_ok else "NO"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
