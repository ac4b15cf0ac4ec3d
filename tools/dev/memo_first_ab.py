"""Dev aid: the vocabulary-seeded memo asked FIRST (option "memo_first", spl_k_pretok.h probe phase) against the memo behind the
vocabulary's tables, in ONE process, the option toggled between blocks of steps: parity vs the oracle, the bench rotations (us per step,
median of the blocks per setting), the first passes after a toggle (the toggle empties the memo: seed + fills), and what creating a seeded
memo costs on the host (memo_ensure: placement, upload, scatter).
   python tools/dev/memo_first_ab.py [label]       (SPL_LIB_PATH selects an A/B build; MEMO_FIRST_AB_QUICK=1: C2 and c2_wide only)"""
import ctypes, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np, torch
from splintr_amd import Tokenizer, corpus, _ffi
from splintr_amd.device import DeviceBatch, encode_device, reserve, result_csr
from oracle.coracle import COracle
label = sys.argv[1] if len(sys.argv) > 1 else os.path.basename(os.environ.get("SPL_LIB_PATH", "default"))
quick = os.environ.get("MEMO_FIRST_AB_QUICK") == "1"
BLOCKS = int(os.environ.get("MEMO_FIRST_AB_BLOCKS", "5"))
L = _ffi.lib(); dev = torch.device("cuda", 0)
L.spl_memo_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
L.spl_memo_seed_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
def opt(tok, k, v):
    if L.spl_set_option(tok.handle, k.encode(), int(v)) != 0: raise RuntimeError(_ffi.last_error())
def stats(tok):
    o = (ctypes.c_uint64 * 4)(); L.spl_memo_stats(tok.handle, o); return list(o)
def seed_stats(tok):
    o = (ctypes.c_uint64 * 2)(); L.spl_memo_seed_stats(tok.handle, o); return list(o)
def packed(texts):
    bs = [t.encode() for t in texts]; off = np.zeros(len(bs) + 1, dtype=np.uint64); np.cumsum([len(b) for b in bs], out=off[1:])
    return np.frombuffer(b"".join(bs), dtype=np.uint8), off
def check(tok, orc, b, t):
    encode_device(tok, b); torch.cuda.synchronize()
    ids, off = result_csr(b); tn, _ = packed(t); o_ids, o_off = orc.encode_packed(tn, b.host_offsets, threads=32)
    return np.array_equal(ids, o_ids) and np.array_equal(off, o_off)
def block(tok, batches, n):
    for i in range(40): encode_device(tok, batches[i % len(batches)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n): encode_device(tok, batches[i % len(batches)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n
stream = torch.cuda.Stream(dev)
with torch.cuda.stream(stream):
    cfgs = [("cl100k_base", "c2", 1002, 1000, 8), ("cl100k_base", "c2_wide", 2002, 1000, 8)]
    if not quick: cfgs += [("o200k_base", "c3", 3003, 250, 4), ("cl100k_base", "c2", 5002, 8000, 1), ("llama3", "c4", 8004, 100000, 1)]
    for vocab, gen, seed, ndocs, nb_ in cfgs:
        orc = COracle(vocab)
        sets = [getattr(corpus, gen)(ndocs, seed=seed + k) for k in range(nb_)]
        batches = [DeviceBatch(t, dev) for t in sets]
        tok = Tokenizer.from_pretrained(vocab)
        reserve(tok, max(b.n_bytes for b in batches) + (1 << 20), 200000)
        n = 400 if ndocs <= 1000 else 30
        res = {0: [], 1: []}; first = {0: [], 1: []}; ok = True
        for blk in range(2 * BLOCKS):
            mf = 1 - blk % 2
            opt(tok, "memo_first", mf)                    # (a change empties the memo: what follows is seed + fills)
            t0 = time.perf_counter()
            for i in range(3 * len(batches) + 4): encode_device(tok, batches[i % len(batches)])
            torch.cuda.synchronize(); first[mf].append((time.perf_counter() - t0) / (3 * len(batches) + 4))
            for i in range(60 * len(batches)): encode_device(tok, batches[i % len(batches)])      # warm: every fill has run
            ok = ok and all(check(tok, orc, b, t) for b, t in zip(batches[:2], sets[:2]))
            res[mf].append(block(tok, batches, n))
        nb = sum(b.n_bytes for b in batches) / len(batches)
        for mf in (1, 0):
            r = sorted(res[mf]); med = r[len(r) // 2]; f = sorted(first[mf])
            print(f"[{label}] {vocab} {gen} x{ndocs} memo_first={mf}: median {med*1e6:9.2f} us/step {nb/med/1e9:6.2f} GB/s  blocks {' '.join('%.2f' % (x * 1e6) for x in res[mf])}  "
                  f"first passes median {f[len(f) // 2]*1e6:9.1f} us/step  {'ok' if ok else 'MISMATCH'}", flush=True)
        print(f"[{label}] {vocab} {gen}: seed {seed_stats(tok)} memo {stats(tok)}", flush=True)
        del tok
# what a seeded memo costs to create (host: placement, upload, one scatter launch per table; the tables' zero fill is in both)
for vocab in ("cl100k_base", "o200k_base"):
    tok = Tokenizer.from_pretrained(vocab)
    tok.encode("warm up")
    for mf in (1, 0, 1, 0, 1, 0):
        opt(tok, "memo_first", mf)
        tok.clear_cache(); torch.cuda.synchronize()
        t0 = time.perf_counter(); tok.encode("warm up"); dt = time.perf_counter() - t0           # the call that builds the memo: tables allocated and zeroed, and the seed
        t0 = time.perf_counter(); tok.encode("warm up"); dt2 = time.perf_counter() - t0
        print(f"[{label}] {vocab} first call behind clear_cache with memo_first={mf}: {dt*1e3:7.2f} ms (the next call {dt2*1e6:6.1f} us)  seed {seed_stats(tok)}", flush=True)
