"""Dev aid: what the headline could gain at best from a cheaper path for two-byte text (profiles/two_byte_words.txt).  The bench's
rotation (cl100k_base, splintr_amd.corpus.c2, seeds 1002 + k, 1000 documents, memo warm) against a CONTROL: the same eight batches with
the eight accented letters C2 holds replaced by their ASCII base letters, so that no word of it leaves the ASCII path of the classify
phase.  The two rotations ALTERNATE, region by region (REGIONS regions of STEPS steps each, timed as bench.py times a region); reported:
the median, lowest and highest region of each, in us per step and MB/s (the control is ~0.3 % shorter: one byte per letter).
   python tools/dev/two_byte_ceiling.py [label]        (SPL_LIB_PATH selects an A/B build; CEILING_REGIONS, default 15; CEILING_STEPS, default 20)
ascii_control() is what tools/dev/gpu_phase_walls.py and gpu_phase_mix.py use for the same control (SPL_ASCII_CONTROL=1)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

LETTERS = str.maketrans("éöñüÅçïã", "eonuAcia")


def ascii_control(texts):
    out = [t.translate(LETTERS) for t in texts]
    assert all(t.isascii() for t in out), "the corpus holds a character beyond the eight letters"
    return out


def main():
    import numpy as np, torch
    from splintr_amd import Tokenizer, corpus
    from splintr_amd.device import DeviceBatch, encode_device, reserve, result_csr
    from oracle.coracle import COracle
    label = sys.argv[1] if len(sys.argv) > 1 else os.path.basename(os.environ.get("SPL_LIB_PATH", "default"))
    REGIONS, STEPS, N_ROT = int(os.environ.get("CEILING_REGIONS", "15")), int(os.environ.get("CEILING_STEPS", "20")), 8
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    sets = [corpus.c2(1000, seed=1002 + k) for k in range(N_ROT)]
    rots = {"rotation": sets, "ascii control": [ascii_control(t) for t in sets]}
    n_letters = sum(len(t) - len(t.translate({c: None for c in LETTERS})) for s in sets for t in s)
    orc = COracle("cl100k_base")
    run = {}
    for name, ts in rots.items():
        tok = Tokenizer.from_pretrained("cl100k_base")
        batches = [DeviceBatch(t, dev) for t in ts]
        reserve(tok, max(b.n_bytes for b in batches), max(b.n_docs for b in batches))
        for p in range(6):                                   # (the chunk memo fills: every batch several times)
            for b in batches: encode_device(tok, b)
        torch.cuda.synchronize()
        ok = True
        for b, t in zip(batches[:2], ts[:2]):
            encode_device(tok, b); torch.cuda.synchronize()
            ids, off = result_csr(b)
            text = np.frombuffer("".join(t).encode(), dtype=np.uint8)
            o_ids, o_off = orc.encode_packed(text, b.host_offsets, threads=16)
            ok = ok and np.array_equal(ids, o_ids) and np.array_equal(off, o_off)
        run[name] = {"tok": tok, "batches": batches, "i": 0, "t": [], "bytes": [], "ok": ok}

    def steps(r, n):
        for _ in range(n):
            encode_device(r["tok"], r["batches"][r["i"] % N_ROT]); r["i"] += 1
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.05:                   # (the GPU's clocks come up under load: bench.py's ramp)
        for r in run.values(): steps(r, 16)
        torch.cuda.synchronize()
    for _ in range(REGIONS):
        for r in run.values():
            steps(r, 5)
            torch.cuda.synchronize()
            i0 = r["i"]; t0 = time.perf_counter()
            steps(r, STEPS)
            torch.cuda.synchronize()
            r["t"].append((time.perf_counter() - t0) / STEPS)
            r["bytes"].append(sum(r["batches"][(i0 + j) % N_ROT].n_bytes for j in range(STEPS)) / STEPS)
    print(f"[{label}] two-byte letters in the rotation: {n_letters} ({n_letters / N_ROT:.0f} per batch); {REGIONS} regions of {STEPS} steps each, alternating", flush=True)
    med = {}
    for name, r in run.items():
        t = sorted(r["t"]); rate = sorted(b / s / 1e6 for b, s in zip(r["bytes"], r["t"]))
        med[name] = t[len(t) // 2]
        print(f"[{label}] {name:14s} median {t[len(t)//2]*1e6:7.2f} us/step (lowest {t[0]*1e6:7.2f}, highest {t[-1]*1e6:7.2f})   median {rate[len(rate)//2]:9.1f} MB/s "
              f"(lowest {rate[0]:9.1f}, highest {rate[-1]:9.1f})   {np.mean(r['bytes']):9.0f} bytes/step   {'bit-exact vs oracle' if r['ok'] else 'MISMATCH'}", flush=True)
    print(f"[{label}] rotation - ascii control: {(med['rotation'] - med['ascii control'])*1e6:6.2f} us per step", flush=True)


if __name__ == "__main__":
    main()
