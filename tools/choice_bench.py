"""Guided choice on the GPU against what a careful caller does today -> profiles/choice_mask.txt.

cl100k_base and o200k_base, B = 256 and 4096 sequences over ONE table of 64 choices (labels and corpus.c2 words), every sequence with 4
or with all 64 of them selected; bursts of STEPS steps with the state carried across them.  A step's ids are the highest allowed id of
every constrained sequence (a sampler that obeys the mask), so a burst finishes its sequences within its first steps and they run free
after that.

  (a) host                the step's ids to the host, per sequence the candidates narrowed by bytes.startswith, the prefixes of every
                          remainder looked up in a dict of the vocabulary's byte strings, a bool mask [B, V] rewritten for the sequences
                          that were constrained, H2D; wall time around the synchronised step
  (b) ChoiceGuide.step    the same step, nothing leaves the GPU; wall time likewise
  (c) the device call     spl_choice_step_device into preallocated outputs, device events around the burst; and, masks only (no ids), the
                          FIRST step's state (every sequence at k = 0, its whole selection alive) against a LATER one (the state behind the
                          burst's first step: one or two slots alive)

The bar: (b) faster than (a) at every shape by more than the two spreads together.  Also: the bytes of constrained rows written per second
by the first-step call, beside DESIGN.md 4.15's fill on the same B -- an observation, not a bar."""
import argparse
import ctypes
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from stop_bench import event_bursts  # noqa: E402
from stream_bench import STEPS, stat, wall_bursts  # noqa: E402
from splintr_amd import Tokenizer, _ffi, corpus  # noqa: E402
from splintr_amd import device as dv  # noqa: E402

LABELS = [" yes", " no", "yes", "no", "positive", "negative", "neutral", " positive", " negative", "A", "B", "C", "D", "true", "false",
          "get_weather", "get_time", "search_web", " maybe", "unknown", "Yes", "No", "yes.", "yesterday"]
HEAL_FILL = {4096: {"cl100k_base": (88.3, 51), "o200k_base": (144.0, 102)}}      # the fill alone, us for MB of mask


def vocabulary(tok):
    """([(id, bytes)] of the ordinary tokens, a special id)"""
    L, out, special = _ffi.lib(), [], None
    p, n = ctypes.c_void_p(), ctypes.c_uint32()
    for i in range(tok.vocab_size):
        kind = L.spl_token_bytes(tok.handle, i, ctypes.byref(p), ctypes.byref(n))
        if kind in (1, 2) and n.value:
            out.append((i, ctypes.string_at(p, n.value)))
        elif kind == 3 and special is None:
            special = i
    return out, special


def choice_strings():
    words = []
    for t in corpus.c2(40):
        for w in t.split():
            if w.isascii() and w.isalpha() and 3 <= len(w) <= 12 and w not in words and w not in LABELS:
                words.append(w)
    return [c.encode() for c in (LABELS + words)[:64]]


class HostGuide:
    """(a): the careful host -- candidate lists, bytes.startswith, a dict of the vocabulary's byte strings, a bool mask per sequence"""

    def __init__(self, toks, choices, end, V, B):
        self.by_id = dict(toks)
        self.by_bytes = {}
        for i, b in toks:
            self.by_bytes.setdefault(b, []).append(i)
        self.choices, self.end, self.V, self.B = choices, end, V, B
        self.mask = np.ones((B, V), dtype=np.bool_)
        self.A, self.k = [[] for _ in range(B)], [0] * B

    def fresh(self, sel):
        for b in range(self.B):
            self.A[b], self.k[b] = list(sel[b]), 0
            self.row(b)

    def row(self, b):
        A, k, m = self.A[b], self.k[b], self.mask[b]
        if not A:
            m[:] = True
            return
        m[:] = False
        for s in A:
            r = self.choices[s][k:]
            if not r:
                m[self.end] = True
            for n in range(1, len(r) + 1):
                for t in self.by_bytes.get(r[:n], ()):
                    m[t] = True

    def step(self, d_ids, dev):
        ids = d_ids.cpu().tolist()
        for b, t in enumerate(ids):
            A, k = self.A[b], self.k[b]
            if not A:
                continue
            tb = self.by_id.get(t)
            S = [s for s in A if self.choices[s].startswith(tb, k)] if tb is not None else []
            if S:
                self.A[b], self.k[b] = S, k + len(tb)
            else:                                                      # END behind a choice that is spelled out, or a break: free either way
                self.A[b] = []
            self.row(b)
        return torch.from_numpy(self.mask).to(dev)


def unpack(mask, V):
    bits = ((mask.unsqueeze(-1) >> torch.arange(32, device=mask.device, dtype=torch.int32)) & 1).reshape(mask.shape[0], -1)
    return bits[:, :V] != 0


def highest_allowed(mask):
    """int64 [B]: the highest id whose bit is set in every row (rows are never all zero)"""
    nw = mask.shape[1]
    last = nw - 1 - (mask != 0).flip(1).to(torch.uint8).argmax(1)
    word = mask.gather(1, last[:, None]).squeeze(1).to(torch.int64) & 0xFFFFFFFF
    return last * 32 + torch.floor(torch.log2(word.to(torch.float64))).to(torch.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--vocabs", default="cl100k_base,o200k_base")
    ap.add_argument("--sizes", default="256,4096")
    ap.add_argument("--selected", default="4,64")
    args = ap.parse_args()
    if not torch.cuda.is_available() or _ffi.lib().spl_device_count() == 0:
        sys.exit("choice_bench: no GPU")
    dev = torch.device("cuda", 0)
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    def line(name, xs):
        med, spread, lo, hi = stat(xs)
        emit(f"  {name:<64} median {med * 1e3:9.2f} us   min {lo * 1e3:9.2f}  max {hi * 1e3:9.2f}  spread {spread * 1e3:8.2f} us   [{len(xs)} bursts]")
        return med, spread

    choices = choice_strings()
    emit(f"choice_bench: {torch.cuda.get_device_name(0)}; library {os.path.basename(_ffi.LIB_PATH)}; one table of {len(choices)} choices (labels and "
         f"corpus.c2 words, {min(map(len, choices))} .. {max(map(len, choices))} bytes); bursts of {STEPS} steps, state carried; per STEP of the batch")
    all_ok, missed = True, []
    for name in args.vocabs.split(","):
        tok = Tokenizer.from_pretrained(name)
        toks, special = vocabulary(tok)
        V = tok.vocab_size
        nw = dv.choice_n_words(tok)
        for B in map(int, args.sizes.split(",")):
            for n_sel in map(int, args.selected.split(",")):
                rng = random.Random(B + n_sel)
                sel = [sorted(rng.sample(range(len(choices)), n_sel)) for _ in range(B)]
                guide = dv.ChoiceGuide(tok, B, choices, end_ids=[special])
                guide.begin(sel)
                state0, mask0 = guide.state.clone(), guide.mask.clone()
                emit()
                emit(f"== {name}, B = {B}, {n_sel} of {len(choices)} choices selected per sequence: V = {V}, n_words = {nw} ({B * nw * 4 / 1e6:.1f} MB of mask), "
                     f"END id {special}")
                script, live_at, alive_at, state1 = [], [], [], None
                for k in range(STEPS):
                    ids = highest_allowed(guide.mask).contiguous()
                    script.append(ids)
                    guide.step(ids)
                    if k == 0:
                        state1 = guide.state.clone()
                    live_at.append(int(guide.live.sum().item()))
                    w0 = guide.state[:, 0].cpu().numpy().view(np.uint64)
                    alive_at.append(round(float(np.mean([bin(int(x)).count("1") for x in w0 if x])) if (w0 != 0).any() else 0.0, 1))
                assert not guide.broken.any().item() and guide.done.all().item(), "the burst does not finish every sequence"
                emit(f"  constrained sequences after each step of the burst: {live_at}")
                emit(f"  slots alive per constrained sequence after each step: {alive_at}")
                host = HostGuide(toks, choices, special, V, B)

                def dev_fresh():
                    guide.state.copy_(state0)
                    guide.mask.copy_(mask0)
                if B <= 256:                                               # the two agree, step for step, on every mask
                    host.fresh(sel)
                    dev_fresh()
                    assert torch.equal(torch.from_numpy(host.mask).to(dev), unpack(mask0, V))
                    for k in range(STEPS):
                        m = host.step(script[k], dev)
                        guide.step(script[k])
                        assert torch.equal(m, unpack(guide.mask, V)), (name, B, n_sel, k)
                w = wall_bursts({"a": (lambda: host.fresh(sel), lambda k: host.step(script[k], dev)),
                                 "b": (dev_fresh, lambda k: guide.step(script[k]))})
                ma, sa = line("(a) host: D2H, startswith, dict lookups, bool mask rows, H2D (wall)", w["a"])
                mb, sb = line("(b) ChoiceGuide.step (wall)", w["b"])
                ok = ma - mb > sa + sb
                all_ok &= ok
                if not ok:
                    missed.append(f"{name} B = {B} selected {n_sel}")
                emit(f"  -> (b) is {ma / mb:.1f}x (a); gain {(ma - mb) * 1e3:.1f} us against the two spreads together {(sa + sb) * 1e3:.1f} us: {'PASS' if ok else 'MISS'}")
                # (c) the call alone
                mask = torch.empty_like(mask0)
                cur = state0.clone()

                def call(state, ids):
                    return dv.choice_step_device(tok, ids, None, state, guide.table, end_ids=[special], mask=mask, state_out=state)
                e = event_bursts({"c": (lambda: cur.copy_(state0), lambda k: call(cur, script[k]))})
                line("(c) spl_choice_step_device, the burst (device events)", e["c"])
                first, later = state0.clone(), state1.clone()
                e = event_bursts({"f": (lambda: None, lambda k: call(first, None)), "l": (lambda: None, lambda k: call(later, None))})
                mf, _ = line(f"(c) masks only, the FIRST step's state ({n_sel} slots alive) (device events)", e["f"])
                n_later = int((state1[:, 0] != 0).sum().item())
                ml, _ = line(f"(c) masks only, a LATER state ({n_later} constrained, {alive_at[0]} slots alive) (device events)", e["l"])
                nbytes = B * nw * 4
                emit(f"  -> first step: {nbytes / 1e6:.1f} MB of constrained rows in {mf * 1e3:.2f} us = {nbytes / (mf * 1e-3) / 1e12:.2f} TB/s; later state: "
                     f"{n_later * nw * 4 / 1e6:.1f} MB constrained + {(B - n_later) * nw * 4 / 1e6:.1f} MB of ones in {ml * 1e3:.2f} us")
                if B in HEAL_FILL and name in HEAL_FILL[B]:
                    us, mb_ = HEAL_FILL[B][name]
                    emit(f"     (DESIGN.md 4.15's fill alone at this B: {us} us for {mb_} MB = {mb_ * 1e6 / (us * 1e-6) / 1e12:.2f} TB/s; its plan comes on top)")
    emit()
    emit(f"(b) faster than (a) at every shape by more than the two spreads together: {'yes' if all_ok else 'NO: ' + '; '.join(missed)}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
