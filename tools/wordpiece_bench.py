#!/usr/bin/env python3
"""Time WordPiece mode (csrc/spl_k_wp.h) on the GPU: device events around bursts of calls, median over the bursts, in this one process.

    python tools/wordpiece_bench.py [--out profiles/wordpiece.txt]

For corpus.c2 (1 000 documents of about 1 KB) and 8 000 documents of the same text (about 8 MB): the normaliser's two passes and the
matcher's two passes (the library's own per-kernel profile), the whole device encode (spl_encode_batch_device) on the WordPiece handle, the same
encode with token spans (spl_encode_batch_spans_device: bytes only, bytes and characters; tools/unigram_bench.py has the same leg),
the same text on a cl100k_base handle, and a device-to-device copy of the same bytes; Hugging Face's tokenizers.encode_batch (wall time)
where that module imports.  The vocabulary is GENERATED -- no real vocab.txt is shipped or needed: up to 30 000 keys (about 21 000 from this corpus), the corpus's
commonest words and word pieces, every character both word-initial and continued."""
import argparse
import collections
import ctypes
import os
import re
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from splintr_amd import Tokenizer, _ffi, corpus  # noqa: E402
from splintr_amd.device import DeviceBatch, encode_device  # noqa: E402


def vocab(texts, size=30000):
    words = collections.Counter(w for t in texts for w in re.findall(r"[^\W_]+", t.lower()))
    chars = sorted({c for t in texts for c in t.lower() if not c.isspace() and c.isprintable()})
    keys = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + chars + ["##" + c for c in chars if c.isalnum()]
    pieces = collections.Counter()
    for w, n in words.items():
        for k in range(2, min(len(w), 8)):
            pieces[w[:k]] += n
            pieces["##" + w[-k:]] += n
    keys += [w for w, _ in words.most_common(size // 2)] + [p for p, _ in pieces.most_common(size)]
    return list(dict.fromkeys(keys))[:size]


def burst_ms(fn, dev, bursts=11, per=8):
    """median over `bursts` of (device time of `per` calls) / per"""
    out = []
    for _ in range(bursts + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        out.append(e0.elapsed_time(e1) / per)
    return statistics.median(out[1:])


def span_legs(tok, batch, dev, plain_ms):
    """The span leg (spl_encode_batch_spans_device into buffers made once): byte spans alone, then byte and character spans, beside the
    plain device encode of the same run."""
    span = [torch.empty((batch.ids.numel(), 2), dtype=torch.int32, device=dev) for _ in range(2)]
    stream = torch.cuda.current_stream(dev).cuda_stream
    lines = []
    for name, c in (("  + byte spans", None), ("  + byte and character spans", span[1].data_ptr())):
        def call():
            rc = _ffi.lib().spl_encode_batch_spans_device(tok.handle, batch.text.data_ptr(), batch.n_bytes, batch.doc_off.data_ptr(), batch.n_docs, 0,
                                                          batch.ids.data_ptr(), batch.ids.numel(), batch.out_off.data_ptr(), span[0].data_ptr(), c, stream)
            assert rc == 0, _ffi.last_error()
        call()
        m = burst_ms(call, dev)
        lines.append(f"   {name:34s} {m:8.4f}   {batch.n_bytes / m / 1e6:.2f} GB/s   {m - plain_ms:+.4f} ms, {m / plain_ms:.2f}x the plain encode")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    L = _ffi.lib()
    keys = vocab(corpus.c2(1000))
    wp = Tokenizer.from_bytes_wordpiece("\n".join(keys).encode() + b"\n")
    cl = Tokenizer.from_pretrained("cl100k_base")
    lines = [f"WordPiece mode, generated vocabulary of {len(keys)} keys (no real vocab.txt is on the machine); ms, median of 11 bursts of 8 calls, device events"]
    for n_docs in (1000, 8000):
        texts = corpus.c2(n_docs)
        batch = DeviceBatch(texts, dev)
        nb = batch.n_bytes
        for t in (wp, cl):
            encode_device(t, batch, False)
        torch.cuda.synchronize(dev)
        n_tok = int(batch.out_off[-1].item())
        lines.append(f"-- corpus.c2, {n_docs} documents, {nb} bytes")
        ms, cnt = (ctypes.c_double * 16)(), (ctypes.c_uint64 * 16)()
        L.spl_profile_enable(wp.handle, 1)
        L.spl_profile_reset(wp.handle)
        for _ in range(20):
            encode_device(wp, batch, False)
        torch.cuda.synchronize(dev)
        L.spl_profile_read(wp.handle, ms, cnt)
        L.spl_profile_enable(wp.handle, 0)
        for i in range(11, 15):
            note = "; with the call's one synchronisation and the bitmap's memset in front" if i == 12 else ""
            lines.append(f"   {L.spl_kernel_name(i).decode():34s} {ms[i] / max(cnt[i], 1):8.4f}   (mean of {cnt[i]} launches{note})")
        src = torch.empty(nb, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        m = burst_ms(lambda: dst.copy_(src), dev)
        lines.append(f"   {'device-to-device copy, same bytes':34s} {m:8.4f}   {nb / m / 1e6:.1f} GB/s")
        for name, t in (("device encode, WordPiece", wp), ("device encode, cl100k_base", cl)):
            m = burst_ms(lambda: encode_device(t, batch, False), dev)
            lines.append(f"   {name:34s} {m:8.4f}   {nb / m / 1e6:.2f} GB/s")
            if t is wp:
                lines += span_legs(wp, batch, dev, m)
        lines.append(f"   ({n_tok} cl100k tokens; every call encodes the same batch again)")
        try:
            import tokenizers as tk
            hf = tk.Tokenizer(tk.models.WordPiece({k: i for i, k in enumerate(keys)}, unk_token="[UNK]"))
            hf.normalizer, hf.pre_tokenizer = tk.normalizers.BertNormalizer(), tk.pre_tokenizers.BertPreTokenizer()
            t0 = time.perf_counter()
            enc = hf.encode_batch(texts, add_special_tokens=False)
            m = (time.perf_counter() - t0) * 1e3
            same = [e.ids for e in enc[:200]] == wp.encode_batch(texts[:200])
            lines.append(f"   {'tokenizers.encode_batch (wall)':34s} {m:8.4f}   {nb / m / 1e6:.3f} GB/s   first 200 documents equal to the device's: {same}")
        except ImportError:
            lines.append("   tokenizers: not installed on this machine")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
