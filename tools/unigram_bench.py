#!/usr/bin/env python3
"""Time Unigram mode (csrc/spl_k_uni.h) on the GPU: device events around bursts of calls, median over the bursts, in this one process.

    python tools/unigram_bench.py [--out profiles/unigram.txt]

For corpus.c2 (1 000 documents of about 1 KB) and 8 000 documents of the same text (about 8 MB): the mode's four phases (the library's
own per-kernel profile), the whole device encode (spl_encode_batch_device) on the Unigram handle, the same text on a WordPiece handle
(tools/wordpiece_bench.py's generated vocabulary), and a device-to-device copy of the same bytes; Hugging Face's tokenizers.encode_batch
of the same Unigram model (wall time) where that module imports.  The vocabulary is GENERATED -- no real model file is shipped or
needed: about 30 000 pieces, the corpus's commonest words (with U+2581 in front) and word pieces and every character, scored by the
logarithm of their relative frequency."""
import argparse
import collections
import ctypes
import math
import os
import re
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from splintr_amd import Tokenizer, _ffi, corpus  # noqa: E402
from splintr_amd.device import DeviceBatch, encode_device  # noqa: E402
from wordpiece_bench import burst_ms, span_legs, vocab as wordpiece_vocab  # noqa: E402

PHASES = ["k_uni_match<count>", "k_uni_long<count>+k_decode_scan", "k_uni_match<write>", "k_uni_long<write>"]


def pieces(texts, size=30000):
    """[(piece, score)]: <unk>, U+2581, every character, the commonest words and word pieces; score = log(count / total)."""
    words = collections.Counter(w for t in texts for w in re.findall(r"\S+", t))
    cnt = collections.Counter()
    for w, n in words.items():
        cnt["▁" + w] += n
        for k in range(1, min(len(w), 8)):
            cnt["▁" + w[:k]] += n
            cnt[w[-k:]] += n
            cnt[w[k:k + 3]] += n
    chars = collections.Counter(c for t in texts for c in t if c not in " \n\r")
    keep = dict(cnt.most_common(size))
    for c, n in chars.items():
        keep[c] = max(keep.get(c, 0), n)
    keep["▁"] = sum(words.values())
    keep = {k: n for k, n in keep.items() if "\n" not in k and "\r" not in k and k != "<unk>" and len(k.encode()) <= 255}
    total = sum(keep.values())
    return [("<unk>", 0.0)] + sorted(((k, math.log(n / total)) for k, n in keep.items()), key=lambda x: -x[1])[:size]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    L = _ffi.lib()
    base = corpus.c2(1000)
    P = pieces(base)
    uni = Tokenizer.from_bytes_unigram(P, 0)
    wp = Tokenizer.from_bytes_wordpiece("\n".join(wordpiece_vocab(base)).encode() + b"\n")
    lines = [f"Unigram mode, generated vocabulary of {len(P)} pieces (no real model file is on the machine); ms, median of 11 bursts of 8 calls, device events"]
    for n_docs in (1000, 8000):
        texts = corpus.c2(n_docs)
        batch = DeviceBatch(texts, dev)
        nb = batch.n_bytes
        for t in (uni, wp):
            encode_device(t, batch, False)
        torch.cuda.synchronize(dev)
        lines.append(f"-- corpus.c2, {n_docs} documents, {nb} bytes")
        ms, cnt = (ctypes.c_double * _ffi.SPL_MAX_KERNELS)(), (ctypes.c_uint64 * _ffi.SPL_MAX_KERNELS)()
        L.spl_profile_enable(uni.handle, 1)
        L.spl_profile_reset(uni.handle)
        for _ in range(20):
            encode_device(uni, batch, False)
        torch.cuda.synchronize(dev)
        L.spl_profile_read(uni.handle, ms, cnt)
        L.spl_profile_enable(uni.handle, 0)
        for k, name in enumerate(PHASES):                    # a Unigram handle counts its phases in slots 11 .. 14
            lines.append(f"   {name:34s} {ms[11 + k] / max(cnt[11 + k], 1):8.4f}   (mean of {cnt[11 + k]} launches)")
        src = torch.empty(nb, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        copy = burst_ms(lambda: dst.copy_(src), dev)
        lines.append(f"   {'device-to-device copy, same bytes':34s} {copy:8.4f}   {nb / copy / 1e6:.1f} GB/s")
        got = {}
        for name, t in (("device encode, Unigram", uni), ("device encode, WordPiece", wp)):
            got[name] = burst_ms(lambda: encode_device(t, batch, False), dev)
            lines.append(f"   {name:34s} {got[name]:8.4f}   {nb / got[name] / 1e6:.2f} GB/s")
            if t is uni:
                lines += span_legs(uni, batch, dev, got[name])
        u =got["device encode, Unigram"]
        lines.append(f"   Unigram / WordPiece on the same bytes: {u / got['device encode, WordPiece']:.2f}x the time; / the copy: {u / copy:.1f}x")
        try:
            import tokenizers as tk
            hf = tk.Tokenizer(tk.models.Unigram([(p, s) for p, s in P], unk_id=0, byte_fallback=False))
            hf.pre_tokenizer = tk.pre_tokenizers.Metaspace(replacement="▁", prepend_scheme="always")
            t0 = time.perf_counter()
            enc = hf.encode_batch(texts, add_special_tokens=False)
            m = (time.perf_counter() - t0) * 1e3
            same = [e.ids for e in enc[:200]] == uni.encode_batch(texts[:200])
            lines.append(f"   {'tokenizers.encode_batch (wall)':34s} {m:8.4f}   {nb / m / 1e6:.3f} GB/s   {m / u:.0f}x the device encode; "
                         f"first 200 documents equal to the device's: {same}")
        except ImportError:
            lines.append("   tokenizers: not installed on this machine")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
