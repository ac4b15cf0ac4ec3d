"""The regex guide on the GPU against what a careful caller does today -> profiles/dfa_mask.txt.

  (i) the index            spl_dfa_index_device for the date, JSON-object and (a|b)*a(a|b){10} patterns (11, about a hundred and 2048
                           states) on cl100k_base and o200k_base: device events around the two launches, and the host compile beside it
  (a) host                 the step's ids to the host, per sequence a Python walk of the ids' bytes through the transition table, the
                           state's row of a bool index [S, V] built beforehand (not timed) copied into a bool mask [B, V], the END bit,
                           H2D; wall time around the synchronised step
  (b) RegexGuide.step      the same step, nothing leaves the GPU; wall time likewise
  (c) the device call      spl_dfa_step_device into preallocated outputs, device events around the burst
  (u) spl_utf8_mask_device the same B and n_words, every sequence at a character boundary: the same gather shape with a fraction of the walk

B = 256 and 4096, K = 1 and 8 ids a step; bursts of STEPS steps with the state carried.  The pattern of the steps is an unbounded JSON
shape and the sampler draws the LOWEST allowed id, so every sequence stays constrained through a burst: every row of every step is a
copied row.  No ratio is a bar here (nothing of this had been measured); the expectation is a step bound by 2 * B * n_words * 4 bytes,
within a small factor of (u)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from choice_bench import unpack, vocabulary  # noqa: E402
from stop_bench import event_bursts  # noqa: E402
from stream_bench import STEPS, stat  # noqa: E402
from splintr_amd import Tokenizer, _ffi, dfa  # noqa: E402
from splintr_amd import device as dv  # noqa: E402

INDEX_PATTERNS = {
    "date": r"\d{4}-\d{2}-\d{2}",
    "json object": r'\{"name": "[^"\\]{1,16}", "score": -?(0|[1-9]\d{0,3})(\.\d{1,2})?, "tags": \[("[a-z]{1,8}"(, "[a-z]{1,8}"){0,3})?\]\}',
    "(a|b)*a(a|b){10}": r"(a|b)*a(a|b){10}",
}
STEP_PATTERN = r'\{"name": "[^"\\]+", "tags": \[("[a-z]+"(, "[a-z]+")*)?\]\}'
KS = (1, 8)


class HostGuide:
    """(a): the careful host -- a transition table, a bool index built beforehand, a Python walk per sequence, a bool mask per sequence"""

    def __init__(self, toks, d, rows_bool, end, V, B):
        self.by_id = dict(toks)
        self.trans, self.accept, self.rows, self.end, self.V, self.B = d.trans.tolist(), d.accept.tolist(), rows_bool, end, V, B
        self.mask = np.ones((B, V), dtype=np.bool_)
        self.q = [0] * B

    def fresh(self):
        for b in range(self.B):
            self.q[b] = 0
            self.row(b)

    def row(self, b):
        q = self.q[b]
        if q < 0:
            self.mask[b] = True
            return
        self.mask[b] = self.rows[q]
        if self.accept[q]:
            self.mask[b, self.end] = True

    def step(self, d_ids, dev):
        ids = d_ids.cpu().tolist()
        for b, row in enumerate(ids):
            q = self.q[b]
            for t in (row if isinstance(row, list) else [row]):
                if q < 0:
                    break
                tb = self.by_id.get(t)
                nq = q
                if tb is None:
                    nq = -1
                else:
                    for x in tb:
                        nq = self.trans[nq][x]
                        if nq == dfa.DEAD:
                            nq = -1
                            break
                q = nq
            self.q[b] = q
            self.row(b)
        return torch.from_numpy(self.mask).to(dev)


def wall_bursts(fresh, step, rounds, warm=1):
    """[ms per step, one per burst]: every burst is STEPS synchronised steps, timed on the host (stream_bench's, with the bursts a parameter:
    the host route at B = 4096 takes half a second a step)"""
    out = []
    for r in range(warm + rounds):
        fresh()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(STEPS):
            step(k)
        torch.cuda.synchronize()
        if r >= warm:
            out.append((time.perf_counter() - t0) * 1e3 / STEPS)
    return out


def lowest_allowed(mask):
    """int64 [B]: the lowest id whose bit is set in every row (rows are never all zero)"""
    first = (mask != 0).to(torch.uint8).argmax(1)
    word = mask.gather(1, first[:, None]).squeeze(1).to(torch.int64) & 0xFFFFFFFF
    low = word & -word
    return first * 32 + torch.round(torch.log2(low.to(torch.float64))).to(torch.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--vocabs", default="cl100k_base,o200k_base")
    ap.add_argument("--sizes", default="256,4096")
    ap.add_argument("--index-rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available() or _ffi.lib().spl_device_count() == 0:
        sys.exit("dfa_bench: no GPU")
    dev = torch.device("cuda", 0)
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    def line(name, xs, unit="us", scale=1e3):
        med, spread, lo, hi = stat(xs)
        emit(f"  {name:<72} median {med * scale:10.2f} {unit}   min {lo * scale:10.2f}  max {hi * scale:10.2f}  spread {spread * scale:9.2f} {unit}   [{len(xs)}]")
        return med, spread

    emit(f"dfa_bench: {torch.cuda.get_device_name(0)}; library {os.path.basename(_ffi.LIB_PATH)}; bursts of {STEPS} steps, state carried; per STEP of the batch")
    summary = []
    for name in args.vocabs.split(","):
        tok = Tokenizer.from_pretrained(name)
        toks, special = vocabulary(tok)
        V = tok.vocab_size
        nw = dv.dfa_n_words(tok)
        dv.dfa_reserve(tok)
        emit()
        emit(f"== {name}: V = {V}, n_words = {nw}, {len(toks)} ordinary ids, END id {special}")
        emit("  (i) the index: compile on the host (wall, once), spl_dfa_index_device (device events around its two launches)")
        for label, pat in INDEX_PATTERNS.items():
            t0 = time.perf_counter()
            d = dfa.compile_regex(pat)
            t_compile = time.perf_counter() - t0
            S = d.n_states
            table = dv.dfa_table(d, dev)
            out = torch.empty(_ffi.SPL_DFA_INDEX_BYTES(S, nw), dtype=torch.uint8, device=dev)
            ms = []
            for r in range(args.index_rounds + 2):
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                dv.dfa_index_device(tok, table, S, n_words=nw, out=out)
                b.record()
                torch.cuda.synchronize()
                if r >= 2:
                    ms.append(a.elapsed_time(b))
            rows, some = dv.dfa_index_rows(out, S, nw)
            bits = int((unpack(rows[:min(S, 64)], 32 * rows.shape[1])).sum().item())
            med, _ = line(f"{label}: {S} states, index {out.numel() / 1e6:.1f} MB, compiled in {t_compile * 1e3:.0f} ms", ms, "ms", 1.0)
            emit(f"     -> {S * len(toks) / (med * 1e-3) / 1e9:.1f} G (state, id) pairs/s; {int(some.sum().item())} states with a row; "
                 f"{bits} bits set in the first {min(S, 64)} rows")
            summary.append(f"index {name} {label}: {S} states {med:.3f} ms")
        # the steps
        d = dfa.compile_regex(STEP_PATTERN)
        emit(f"  the steps: {STEP_PATTERN!r}: {d.n_states} states; the sampler draws the lowest allowed id")
        for B in map(int, args.sizes.split(",")):
            guide = dv.RegexGuide(tok, B, d, end_ids=[special])
            guide.begin()
            state0, mask0 = guide.state.clone(), guide.mask.clone()
            flat = []
            for k in range(STEPS * max(KS)):
                ids = lowest_allowed(guide.mask).contiguous()
                flat.append(ids)
                guide.step(ids)
            assert guide.live.all().item() and not guide.broken.any().item(), "a sequence left its constraint inside the burst"
            rows_t, _ = dv.dfa_index_rows(guide.index, guide.n_states, guide.n_words)
            rows_bool = unpack(rows_t, V).cpu().numpy()
            u_state = torch.zeros(B, dtype=torch.int64, device=dev)
            u_mask = torch.empty_like(mask0)
            dv.utf8_mask_reserve(tok)
            for K in KS:
                script = [torch.stack(flat[k * K:(k + 1) * K], dim=1).contiguous() if K > 1 else flat[k] for k in range(STEPS)]
                emit()
                emit(f"  -- {name}, B = {B}, K = {K}: {B * nw * 4 / 1e6:.1f} MB of mask a step")
                host = HostGuide(toks, d, rows_bool, special, V, B)

                def dev_fresh():
                    guide.state.copy_(state0)
                    guide.mask.copy_(mask0)
                if B <= 256:                                               # the two agree, step for step, on every mask
                    host.fresh()
                    dev_fresh()
                    assert torch.equal(torch.from_numpy(host.mask).to(dev), unpack(mask0, V))
                    for k in range(STEPS):
                        m = host.step(script[k], dev)
                        guide.step(script[k])
                        assert torch.equal(m, unpack(guide.mask, V)), (name, B, K, k)
                wa = wall_bursts(host.fresh, lambda k: host.step(script[k], dev), rounds=5 if B <= 256 else 2)
                wb = wall_bursts(dev_fresh, lambda k: guide.step(script[k]), rounds=21, warm=3)
                ma, sa = line("(a) host: D2H, a Python walk, bool index rows, H2D (wall)", wa)
                mb, sb = line("(b) RegexGuide.step (wall)", wb)
                emit(f"  -> (b) is {ma / mb:.1f}x (a); gain {(ma - mb) * 1e3:.1f} us against the two spreads together {(sa + sb) * 1e3:.1f} us")
                mask = torch.empty_like(mask0)
                cur = state0.clone()
                live = torch.empty(B, dtype=torch.uint8, device=dev)

                def call(k):
                    dv.dfa_step_device(tok, script[k], None, cur, guide.table, guide.index, end_ids=[special], n_states=guide.n_states, mask=mask,
                                       state_out=cur, live=live)
                e = event_bursts({"c": (lambda: cur.copy_(state0), call),
                                  "u": (lambda: None, lambda k: dv.utf8_mask_device(tok, u_state, out=u_mask))})
                mc, _ = line("(c) spl_dfa_step_device, the burst (device events)", e["c"])
                mu, _ = line("(u) spl_utf8_mask_device, same B and n_words (device events)", e["u"])
                nbytes = 2 * B * nw * 4
                emit(f"  -> (c): {nbytes / 1e6:.1f} MB read and written in {mc * 1e3:.2f} us = {nbytes / (mc * 1e-3) / 1e12:.2f} TB/s; (c) is {mc / mu:.2f}x (u)")
                summary.append(f"step {name} B={B} K={K}: host {ma * 1e3:.0f} us, RegexGuide.step {mb * 1e3:.1f} us, call {mc * 1e3:.1f} us, utf8 mask {mu * 1e3:.1f} us, "
                               f"call/utf8 {mc / mu:.2f}")
    emit()
    emit("summary")
    for s in summary:
        emit("  " + s)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
