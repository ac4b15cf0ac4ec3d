"""Token healing on the GPU against what a careful caller does today -> profiles/token_mask.txt.

cl100k_base and o200k_base, B = 256 and 4096 prompts (corpus.c2 texts cut inside a word, so |P| is what real cut prompts give), begin with
auto and max_back 3, then bursts of STEPS steps with the state carried across them; a step's ids are the highest allowed id of every
constrained sequence (a sampler that obeys the mask), so a burst heals its sequences within its first steps and runs free after that.

  (a) host                the step's ids to the host, per sequence the pending prefix against a SORTED list of the vocabulary's byte strings
                          (bisect for the covering range, a loop over the prefix for the partial tokens), a bool mask [B, V] built per
                          sequence, H2D; wall time around the synchronised step
  (b) TokenHealer.step    the same step, nothing leaves the GPU; wall time likewise
  (c) the device call     spl_heal_step_device into preallocated outputs, device events around the burst; and on the begin state (every
                          rolled-back sequence constrained) the plan and the fill alone ("heal_phase")
  (d) (c) with KEEP_FREE  once every sequence is free: the call writes nothing

The bar: (b) faster than (a) at every shape by more than the two spreads together.  Also: the fill's bytes per second against the HBM
roofline, and the plan's time over the sequence count."""
import argparse
import bisect
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from stop_bench import event_bursts  # noqa: E402
from stream_bench import STEPS, stat, wall_bursts  # noqa: E402
from splintr_amd import Tokenizer, _ffi, corpus  # noqa: E402
from splintr_amd import device as dv  # noqa: E402

HBM_PEAK = 8.0e12          # bytes per second, MI355X (8 TB/s)


def vocabulary(tok):
    """[(id, bytes)] of the ordinary tokens"""
    L, out = _ffi.lib(), []
    p, n = ctypes.c_void_p(), ctypes.c_uint32()
    for i in range(tok.vocab_size):
        if L.spl_token_bytes(tok.handle, i, ctypes.byref(p), ctypes.byref(n)) in (1, 2) and n.value:
            out.append((i, ctypes.string_at(p, n.value)))
    return out


def cut_prompts(B):
    out = []
    for k, t in enumerate(corpus.c2(B)):
        cuts = [c for c in range(8, min(len(t), 200)) if t[c - 1].isascii() and t[c - 1].isalpha() and t[c].isascii() and t[c].isalpha()]
        out.append(t[:cuts[(13 * k) % len(cuts)]] if cuts else t[:8])
    return out


class HostHealer:
    """(a): the trie-free careful host -- sorted byte strings, bisect, a bool mask per sequence"""

    def __init__(self, toks, V, B):
        order = sorted(range(len(toks)), key=lambda r: toks[r][1])
        self.keys = [toks[r][1] for r in order]
        self.ids = np.array([toks[r][0] for r in order], dtype=np.int64)
        self.by_id = dict(toks)
        self.by_bytes = {b: i for i, b in toks}
        self.V, self.B = V, B
        self.mask = np.ones((B, V), dtype=np.bool_)
        self.P = [b""] * B

    def fresh(self, prefixes):
        self.P = list(prefixes)
        for b in range(self.B):
            self.row(b)

    def row(self, b):
        P, m = self.P[b], self.mask[b]
        if not P:
            m[:] = True
            return
        m[:] = False
        lo = bisect.bisect_left(self.keys, P)
        hi = lo
        q = P.rstrip(b"\xff")                                            # the smallest string above everything that starts with P
        hi = bisect.bisect_left(self.keys, q[:-1] + bytes([q[-1] + 1]), lo) if q else len(self.keys)
        m[self.ids[lo:hi]] = True
        for k in range(1, len(P)):
            t = self.by_bytes.get(P[:k])
            if t is not None:
                m[t] = True

    def step(self, d_ids, dev):
        ids = d_ids.cpu().tolist()
        for b, t in enumerate(ids):
            P = self.P[b]
            if not P:
                continue
            tb = self.by_id.get(t)
            if tb is None:
                P = b""
            elif tb.startswith(P):
                P = b""
            elif P.startswith(tb):
                P = P[len(tb):]
            else:
                P = b""
            self.P[b] = P
            self.row(b)
        return torch.from_numpy(self.mask).to(dev)


def unpack(mask, V):
    bits = ((mask.unsqueeze(-1) >> torch.arange(32, device=mask.device, dtype=torch.int32)) & 1).reshape(mask.shape[0], -1)
    return bits[:, :V] != 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--vocabs", default="cl100k_base,o200k_base")
    ap.add_argument("--sizes", default="256,4096")
    args = ap.parse_args()
    if not torch.cuda.is_available() or _ffi.lib().spl_device_count() == 0:
        sys.exit("heal_bench: no GPU")
    dev = torch.device("cuda", 0)
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    def line(name, xs):
        med, spread, lo, hi = stat(xs)
        emit(f"  {name:<56} median {med * 1e3:9.2f} us   min {lo * 1e3:9.2f}  max {hi * 1e3:9.2f}  spread {spread * 1e3:8.2f} us   [{len(xs)} bursts]")
        return med, spread

    L = _ffi.lib()
    emit(f"heal_bench: {torch.cuda.get_device_name(0)}; library {os.path.basename(_ffi.LIB_PATH)}; prompts: corpus.c2 texts cut inside a word, "
         f"begin auto, max_back 3; bursts of {STEPS} steps, state carried; per STEP of the batch unless said otherwise")
    all_ok = True
    for name in args.vocabs.split(","):
        tok = Tokenizer.from_pretrained(name)
        toks = vocabulary(tok)
        V = tok.vocab_size
        nw = dv.heal_n_words(tok)
        for B in map(int, args.sizes.split(",")):
            enc = tok.encode_batch(cut_prompts(B))
            K = max(len(e) for e in enc)
            rows = torch.zeros((B, K), dtype=torch.int64)
            for b, e in enumerate(enc):
                rows[b, :len(e)] = torch.tensor(e, dtype=torch.int64)
            rows, lens = rows.to(dev), torch.tensor([len(e) for e in enc], dtype=torch.int32, device=dev)
            healer = dv.TokenHealer(tok, B, max_back=3, auto=True)
            healer.begin(rows, lens)
            state0, mask0 = healer.state.clone(), healer.mask.clone()
            pend = healer.pending.cpu().numpy()
            raw = state0.cpu().numpy().view(np.uint64)
            prefixes = [raw[b, 1:].astype("<u8").tobytes()[:pend[b]] for b in range(B)]
            emit()
            emit(f"== {name}, B = {B}: V = {V}, n_words = {nw} ({B * nw * 4 / 1e6:.1f} MB of mask); {int((pend > 0).sum())} prompts rolled back, "
                 f"|P| median {int(np.median(pend[pend > 0])) if (pend > 0).any() else 0} max {int(pend.max())} bytes")
            # the burst's ids: a sampler that obeys the mask (the highest allowed id: mostly a covering token); free sequences draw id 0
            script, live_at = [], []
            for k in range(STEPS):
                last = 32 * nw - 1 - unpack(healer.mask, 32 * nw).to(torch.uint8).flip(1).argmax(1)
                ids = torch.where(healer.live != 0, last, torch.zeros_like(last)).contiguous()
                script.append(ids)
                healer.step(ids)
                live_at.append(int(healer.n[0].item()))
            emit(f"  constrained sequences after each step of the burst: {live_at}")
            host = HostHealer(toks, V, B)

            def dev_fresh():
                healer.state.copy_(state0)
                healer.mask.copy_(mask0)
            if B <= 256:                                                   # the two agree, step for step
                host.fresh(prefixes)
                dev_fresh()
                assert torch.equal(torch.from_numpy(host.mask).to(dev), unpack(mask0, V))
                for k in range(STEPS):
                    m = host.step(script[k], dev)
                    healer.step(script[k])
                    assert torch.equal(m, unpack(healer.mask, V)), (name, B, k)
            w = wall_bursts({"a": (lambda: host.fresh(prefixes), lambda k: host.step(script[k], dev)),
                             "b": (dev_fresh, lambda k: healer.step(script[k]))})
            ma, sa = line("(a) host: D2H, bisect, bool mask per sequence, H2D (wall)", w["a"])
            mb, sb = line("(b) TokenHealer.step (wall)", w["b"])
            ok = ma - mb > sa + sb
            all_ok &= ok
            emit(f"  -> (b) is {ma / mb:.1f}x (a); gain {(ma - mb) * 1e3:.1f} us against the two spreads together {(sa + sb) * 1e3:.1f} us: {'PASS' if ok else 'MISS'}")
            # (c) the call alone
            st_out, mask, live, n = torch.empty_like(state0), torch.empty_like(mask0), None, None
            cur = state0.clone()

            def call(state, ids, keep=False, m=mask):
                return dv.heal_step_device(tok, ids, None, state, keep_free=keep, mask=m, state_out=state)

            def c_fresh():
                cur.copy_(state0)
            e = event_bursts({"c": (c_fresh, lambda k: call(cur, script[k]))})
            mc, _ = line("(c) spl_heal_step_device, the burst (device events)", e["c"])
            fixed = state0.clone()
            res = {}
            for phase, what in ((0, "plan + fill"), (1, "plan alone"), (2, "fill alone")):
                assert L.spl_set_option(tok.handle, b"heal_phase", phase) == 0
                e = event_bursts({"x": (lambda: None, lambda k: call(fixed, None))})
                res[phase], _ = line(f"(c) the masks of the begin state, {what} (device events)", e["x"])
            assert L.spl_set_option(tok.handle, b"heal_phase", 0) == 0
            nbytes = B * nw * 4
            emit(f"  -> fill alone: {nbytes / (res[2] * 1e-3) / 1e12:.2f} TB/s of mask written, {100 * nbytes / (res[2] * 1e-3) / HBM_PEAK:.0f} % of the "
                 f"{HBM_PEAK / 1e12:.0f} TB/s roofline; plan alone {res[1] * 1e3:.2f} us for {B} sequences")
            free = torch.zeros_like(state0)
            ones = torch.full_like(mask0, -1)
            e = event_bursts({"f": (lambda: None, lambda k: call(free, script[-1])),
                              "d": (lambda: None, lambda k: call(free, script[-1], keep=True, m=ones))})
            mf, _ = line("(c) every sequence free: ones written (device events)", e["f"])
            md, _ = line("(d) every sequence free, KEEP_FREE: nothing written", e["d"])
            emit(f"  -> the ones: {nbytes / (mf * 1e-3) / 1e12:.2f} TB/s, {100 * nbytes / (mf * 1e-3) / HBM_PEAK:.0f} % of the roofline; KEEP_FREE saves {(mf - md) * 1e3:.2f} us a step")
            assert (ones == -1).all().item()
        if name == args.vocabs.split(",")[0]:
            emit()
            emit(f"== {name}: the plan alone over the sequence count (every sequence constrained: the begin states above, repeated), device events")
            L.spl_set_option(tok.handle, b"heal_phase", 1)
            live_rows = state0[(state0[:, 0] & 0x7F) != 0]
            for n_seq in (16, 64, 256, 1024, 4096, 16384):
                st = live_rows.repeat((n_seq + live_rows.shape[0] - 1) // live_rows.shape[0], 1)[:n_seq].contiguous()
                m = torch.empty((n_seq, nw), dtype=torch.int32, device=dev)
                e = event_bursts({"p": (lambda: None, lambda k: dv.heal_step_device(tok, None, None, st, mask=m, state_out=st))})
                med, spread, _, _ = stat(e["p"])
                emit(f"  B = {n_seq:6d}   plan {med * 1e3:8.2f} us (spread {spread * 1e3:6.2f})   {med * 1e3 / n_seq * 1e3:8.1f} ns a sequence")
            L.spl_set_option(tok.handle, b"heal_phase", 0)
    emit()
    emit(f"(b) faster than (a) at every shape by more than the two spreads together: {'yes' if all_ok else 'NO'}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
