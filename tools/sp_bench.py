#!/usr/bin/env python3
"""Time SentencePiece mode (csrc/spl_k_sp.h) on the GPU: three comparisons, medians over repeated calls in this one process.

    python tools/sp_bench.py [--out profiles/sp_encode.txt]

  1  the two rewrite launches (count pass + scan, write pass; the library's own per-kernel profile, device events) beside a
     device-to-device copy of the same input bytes;
  2  the whole device encode (spl_encode_batch_device) of an English corpus on a SentencePiece handle beside the same corpus on a
     custom-pattern handle with [^\\s]+|\\s+ and the same vocabulary -- different ids, the cost comparison;
  3  the host-to-host call (encode_batch_csr) on the SentencePiece handle.
The vocabulary: cl100k_base's keys with their leading space spelled U+2581, plus the marker and its first two bytes, as tiktoken text."""
import argparse
import base64
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from oracle.pyoracle import load_splv  # noqa: E402
from splintr_amd import SENTENCEPIECE_PATTERN, Tokenizer, _ffi, corpus  # noqa: E402
from splintr_amd.device import DeviceBatch, encode_device  # noqa: E402

MARK = "▁".encode()


def vocab():
    enc, _ = load_splv(os.path.join(os.path.dirname(os.path.abspath(_ffi.__file__)), "data", "cl100k_base.splv"))
    keys, nxt = {}, max(enc.values()) + 1
    for k, r in enc.items():
        keys.setdefault(MARK + k[1:] if k[:1] == b" " and len(k) > 1 else k, r)
    for k in (MARK[:2], MARK):
        if k not in keys:
            keys[k], nxt = nxt, nxt + 1
    return b"".join(base64.b64encode(k) + b" %d\n" % r for k, r in keys.items())


def timed(fn, reps, sync):
    out = []
    for _ in range(reps):
        sync()
        t = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out[2:]), min(out[2:]), max(out[2:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--docs", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=23)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    blob, texts = vocab(), corpus.c2(a.docs)
    sp = Tokenizer.from_bytes_sentencepiece(blob, SENTENCEPIECE_PATTERN)
    cu = Tokenizer.from_bytes(blob, SENTENCEPIECE_PATTERN)
    nbytes = sum(len(t.encode()) for t in texts)
    lines = [f"SentencePiece mode, {a.docs} documents of corpus.c2, {nbytes} bytes; median (min .. max) of {a.reps - 2} calls, ms"]
    L = _ffi.lib()
    batch = DeviceBatch(texts, dev)
    enc = {n: (lambda t=t: encode_device(t, batch, False)) for n, t in (("sentencepiece", sp), ("custom [^\\s]+|\\s+", cu))}
    for fn in enc.values():
        fn()
    # 1: the rewrite launches, from the per-kernel profile
    ms, cnt = (ctypes.c_double * 16)(), (ctypes.c_uint64 * 16)()
    L.spl_profile_enable(sp.handle, 1)
    L.spl_profile_reset(sp.handle)
    for _ in range(a.reps):
        enc["sentencepiece"]()
    sync()
    L.spl_profile_read(sp.handle, ms, cnt)
    L.spl_profile_enable(sp.handle, 0)
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    cp = timed(lambda: dst.copy_(src), a.reps, sync)
    for i in (9, 10):
        lines.append(f"1  {L.spl_kernel_name(i).decode():38s} {ms[i] / max(cnt[i], 1):8.4f}   (mean of {cnt[i]} launches, device events)")
    lines.append(f"1  {'device-to-device copy, same bytes':38s} {cp[0]:8.4f}   ({cp[1]:.4f} .. {cp[2]:.4f}; host-timed, includes the launch)")
    # 2: the whole device encode
    for n, fn in enc.items():
        m = timed(fn, a.reps, sync)
        lines.append(f"2  device encode, {n:22s} {m[0]:8.4f}   ({m[1]:.4f} .. {m[2]:.4f})   {nbytes / m[0] / 1e6:.2f} GB/s")
    # 3: host to host
    m = timed(lambda: sp.encode_batch_csr(texts), a.reps, sync)
    lines.append(f"3  host-to-host encode_batch_csr, sentencepiece {m[0]:8.4f}   ({m[1]:.4f} .. {m[2]:.4f})   {nbytes / m[0] / 1e6:.2f} GB/s")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
