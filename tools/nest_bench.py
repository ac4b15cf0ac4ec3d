"""JSON mode on the GPU against the regex guide's step and against what a careful caller does today ->
profiles/nest_mask.txt.

  (i) the index            spl_nest_index_device for json_table() on cl100k_base and o200k_base: wall time around the call (it
                           synchronises once to read n_dep), n_dep and the longest dep list
  (s) inside strings       every sequence sits in a string of a nested array: the state has no dependent id, the step is the regex guide's
                           row copy
  (v) value boundaries     every sequence spells 1,1,1, ... four brackets deep: it lands behind a number and behind a comma, the two kinds of
                           state with the longest dep lists (closers; openers and numbers that run into a closer)
  (d) spl_dfa_step_device  the regex guide on the unbounded JSON shape of tools/dfa_bench.py, the lowest allowed id drawn: MEASURED IN THE
                           SAME RUN, twice, so that its own repeated medians say what a difference means
  (z) the ops-zero table   nest.from_dfa of (d)'s automaton through spl_nest_step_device on (d)'s script
  (h) host                 what the device call replaces: the step's ids to the host, per sequence a Python walk over (state, stack), the
                           state's bool row and its dependent ids walked against the stack, a bool mask [B, V], H2D -- B = 256 only

B = 256 and 4096, K = 1 and 8 ids a step; bursts of STEPS steps with the state carried; device events around the burst for the bare calls,
wall time for NestGuide.step and the host.  No number here is a bar: none existed."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from choice_bench import unpack, vocabulary  # noqa: E402
from dfa_bench import STEP_PATTERN, lowest_allowed, wall_bursts  # noqa: E402
from stop_bench import event_bursts  # noqa: E402
from stream_bench import STEPS, stat  # noqa: E402
from splintr_amd import Tokenizer, _ffi, dfa, nest  # noqa: E402
from splintr_amd import device as dv  # noqa: E402

KS = (1, 8)
DEPTH = 4


class HostNest:
    """(h): the careful host -- the table as lists, a bool index built beforehand, a Python walk per sequence, a bool mask per sequence"""

    def __init__(self, toks, t, rows_bool, deps, end, V, B, max_depth):
        self.by_id, self.t, self.rows, self.deps, self.end, self.V, self.B, self.max_depth = dict(toks), t, rows_bool, deps, end, V, B, max_depth
        self.mask = np.ones((B, V), dtype=np.bool_)
        self.at = [None] * B
        self.trans, self.op, self.ret, self.S = t.trans.tolist(), t.op.tolist(), t.ret.tolist(), t.n_states

    def walk(self, q, stack, data):
        """NestTable.walk over lists"""
        for x in data:
            v, o = self.trans[q][x], self.op[q][x]
            if o == 0:
                if v >= self.S:
                    return None
                q = v
            elif o & 0xF0 == nest.PUSH:
                if v >= self.S or len(stack) >= self.max_depth:
                    return None
                q, stack = v, stack + (o & 15,)
            elif o == nest.POP and stack and v < len(self.ret) and self.ret[v][stack[-1]] < self.S:
                q, stack = self.ret[v][stack[-1]], stack[:-1]
            else:
                return None
        return q, stack

    def fresh(self, at):
        self.at = list(at)
        for b in range(self.B):
            self.row(b)

    def row(self, b):
        if self.at[b] is None:
            self.mask[b] = True
            return
        q, stack = self.at[b]
        self.mask[b] = self.rows[q]
        for i in self.deps[q]:
            if self.walk(q, stack, self.by_id[i]) is not None:
                self.mask[b, i] = True
        if self.t.ends(q, stack):
            self.mask[b, self.end] = True

    def step(self, d_ids, dev):
        ids = d_ids.cpu().tolist()
        for b, row in enumerate(ids):
            for i in (row if isinstance(row, list) else [row]):
                if self.at[b] is None:
                    break
                tb = self.by_id.get(i)
                self.at[b] = self.walk(self.at[b][0], self.at[b][1], tb) if tb is not None else None
            self.row(b)
        return torch.from_numpy(self.mask).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--vocabs", default="cl100k_base,o200k_base")
    ap.add_argument("--sizes", default="256,4096")
    ap.add_argument("--index-rounds", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip (h)")
    args = ap.parse_args()
    if not torch.cuda.is_available() or _ffi.lib().spl_device_count() == 0:
        sys.exit("nest_bench: no GPU")
    dev = torch.device("cuda", 0)
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    def line(name, xs, unit="us", scale=1e3):
        med, spread, lo, hi = stat(xs)
        emit(f"  {name:<78} median {med * scale:10.2f} {unit}   min {lo * scale:10.2f}  max {hi * scale:10.2f}  spread {spread * scale:9.2f} {unit}   [{len(xs)}]")
        return med, spread

    emit(f"nest_bench: {torch.cuda.get_device_name(0)}; library {os.path.basename(_ffi.LIB_PATH)}; bursts of {STEPS} steps, state carried; per STEP of the batch")
    summary = []
    t_json = nest.json_table()
    d_shape = dfa.compile_regex(STEP_PATTERN)
    for name in args.vocabs.split(","):
        tok = Tokenizer.from_pretrained(name)
        toks, special = vocabulary(tok)
        one = {b: i for i, b in toks if len(b) == 1}
        V = tok.vocab_size
        nw = dv.dfa_n_words(tok)
        dv.nest_reserve(tok)
        emit()
        emit(f"== {name}: V = {V}, n_words = {nw}, {len(toks)} ordinary ids, END id {special}")
        table = dv.nest_table(t_json, dev)
        S = t_json.n_states
        ms, n_dep = [], 0
        for r in range(args.index_rounds + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            index, n_dep = dv.nest_index_device(tok, table, S, 1, n_words=nw, dep_cap=1 << 16)
            torch.cuda.synchronize()
            if r:
                ms.append((time.perf_counter() - t0) * 1e3)
        _, dep_off, _, some = dv.nest_index_views(index, S, nw, n_dep)
        lens = (dep_off[1:] - dep_off[:-1]).cpu().numpy()
        med, _ = line(f"(i) json_table(): {S} states, index {index.numel() / 1e6:.1f} MB, dep_cap 65536 given (wall, one synchronisation inside)", ms, "ms", 1.0)
        emit(f"     -> n_dep {n_dep}; the longest dep list {int(lens.max())} (state {int(lens.argmax())}), {int((lens == 0).sum())} states with none; "
             f"{S * len(toks) / (med * 1e-3) / 1e9:.1f} G (state, id) pairs/s")
        summary.append(f"index {name}: {S} states, n_dep {n_dep}, longest {int(lens.max())}, {med:.3f} ms")
        for B in map(int, args.sizes.split(",")):
            guide = dv.NestGuide(tok, B, t_json, end_ids=[special], max_depth=32)
            rx = dv.RegexGuide(tok, B, d_shape, end_ids=[special])
            zero = dv.NestGuide(tok, B, nest.from_dfa(d_shape), end_ids=[special])
            rx.begin()
            rx_state0 = rx.state.clone()
            flat = []
            for k in range(STEPS * max(KS)):
                ids = lowest_allowed(rx.mask).contiguous()
                flat.append(ids)
                rx.step(ids)
            assert rx.live.all().item(), "a sequence left its constraint inside the burst"
            zero.begin()
            z_state0 = zero.state.clone()

            def opened(first):
                guide.begin()
                for x in first:
                    guide.step(torch.full((B,), one[x], dtype=torch.int64, device=dev))
                assert guide.live.all().item()
                return guide.state.clone()
            s_state0 = opened([b"["] * DEPTH + [b'"'])
            v_state0 = opened([b"["] * DEPTH)
            col = lambda x: torch.full((B,), one[x], dtype=torch.int64, device=dev)
            for K in KS:
                emit()
                emit(f"  -- {name}, B = {B}, K = {K}: {B * nw * 4 / 1e6:.1f} MB of mask a step")
                rx_script = [torch.stack(flat[k * K:(k + 1) * K], dim=1).contiguous() if K > 1 else flat[k] for k in range(STEPS)]
                # (v): 1 , 1 , ... -- K = 1 lands behind a number and behind a comma in turns, K = 8 behind a comma every step
                s_script = [col(b"a") if K == 1 else torch.stack([col(b"a")] * K, dim=1).contiguous()] * STEPS
                v_script = [(col(b"1") if k % 2 == 0 else col(b",")) if K == 1 else torch.stack([col(b"1"), col(b",")] * (K // 2), dim=1).contiguous()
                            for k in range(STEPS)]
                mask = torch.empty((B, nw), dtype=torch.int32, device=dev)
                live = torch.empty(B, dtype=torch.uint8, device=dev)
                cur = {n_: s.clone() for n_, s in (("s", s_state0), ("v", v_state0), ("z", z_state0), ("d", rx_state0), ("e", rx_state0))}

                def nest_call(g, key, script):
                    return lambda k: dv.nest_step_device(tok, script[k], None, cur[key], g.table, g.index, n_states=g.n_states, n_ret=g.n_ret, dep_cap=g.n_dep,
                                                         end_ids=[special], max_depth=g.max_depth, mask=mask, state_out=cur[key], live=live)

                def dfa_call(key):
                    return lambda k: dv.dfa_step_device(tok, rx_script[k], None, cur[key], rx.table, rx.index, end_ids=[special], n_states=rx.n_states, mask=mask,
                                                        state_out=cur[key], live=live)
                e = event_bursts({"d": (lambda: cur["d"].copy_(rx_state0), dfa_call("d")),
                                  "s": (lambda: cur["s"].copy_(s_state0), nest_call(guide, "s", s_script)),
                                  "v": (lambda: cur["v"].copy_(v_state0), nest_call(guide, "v", v_script)),
                                  "z": (lambda: cur["z"].copy_(z_state0), nest_call(zero, "z", rx_script)),
                                  "e": (lambda: cur["e"].copy_(rx_state0), dfa_call("e"))})
                assert live.all().item(), "a sequence left its constraint inside the burst"
                md, _ = line("(d) spl_dfa_step_device, the unbounded JSON shape (device events)", e["d"])
                me, _ = line("(d) again, the same call in the same run", e["e"])
                mz, _ = line("(z) spl_nest_step_device, the ops-zero table of (d) on (d)'s ids", e["z"])
                ms_, _ = line("(s) spl_nest_step_device, json_table(), inside strings (no dependent id)", e["s"])
                mv, _ = line("(v) spl_nest_step_device, json_table(), value boundaries (the longest dep lists)", e["v"])
                nbytes = 2 * B * nw * 4
                emit(f"  -> {nbytes / 1e6:.1f} MB read and written a step: (d) {nbytes / (md * 1e-3) / 1e12:.2f} TB/s, (s) {nbytes / (ms_ * 1e-3) / 1e12:.2f} TB/s, "
                     f"(v) {nbytes / (mv * 1e-3) / 1e12:.2f} TB/s; (z) - (d) = {(mz - md) * 1e3:+.2f} us against (d)'s two medians {abs(md - me) * 1e3:.2f} us apart")

                def g_fresh(state0):
                    return lambda: guide.state.copy_(state0)
                ws = wall_bursts(g_fresh(s_state0), lambda k: guide.step(s_script[k]), rounds=11, warm=2)
                wv = wall_bursts(g_fresh(v_state0), lambda k: guide.step(v_script[k]), rounds=11, warm=2)
                mws, _ = line("(s) NestGuide.step (wall)", ws)
                mwv, _ = line("(v) NestGuide.step (wall)", wv)
                row = f"step {name} B={B} K={K}: dfa {md * 1e3:.1f} / {me * 1e3:.1f} us, ops-zero {mz * 1e3:.1f} us, strings {ms_ * 1e3:.1f} us, values {mv * 1e3:.1f} us, " \
                      f"NestGuide.step {mws * 1e3:.1f} / {mwv * 1e3:.1f} us"
                if B <= 256 and not args.no_host:
                    rows_t, dep_off_t, dep_ids_t, _ = dv.nest_index_views(guide.index, guide.n_states, nw, guide.n_dep)
                    rows_bool = unpack(rows_t, V).cpu().numpy()
                    off, dep = dep_off_t.cpu().tolist(), dep_ids_t.cpu().tolist()
                    deps = [dep[off[q]:off[q + 1]] for q in range(guide.n_states)]
                    host = HostNest(toks, nest.NestTable(t_json.trans, t_json.op, t_json.ret, t_json.accept), rows_bool, deps, special, V, B, guide.max_depth)
                    at0 = [t_json.walk(0, (), b"[" * DEPTH, 32)] * B
                    host.fresh(at0)                                                # the two agree, step for step, on every mask
                    guide.state.copy_(v_state0)
                    for k in range(4):
                        m = host.step(v_script[k], dev)
                        guide.step(v_script[k])
                        assert torch.equal(m, unpack(guide.mask, V)), (name, B, K, k)
                    wh = []
                    for k in range(4, 8):                                          # (a step takes a second: four of them, not a burst)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        host.step(v_script[k], dev)
                        torch.cuda.synchronize()
                        wh.append((time.perf_counter() - t0) * 1e3)
                    mh, _ = line("(h) host at value boundaries: D2H, a Python walk, bool rows, the dep ids walked, H2D (wall, single steps)", wh)
                    emit(f"  -> (v) NestGuide.step is {mh / mwv:.0f}x (h)")
                    row += f", host {mh * 1e3:.0f} us"
                summary.append(row)
    emit()
    emit("not measured: a batch spread over many states' rows (every sequence of a burst reads the same one or two rows here, so the row reads hit the")
    emit("cache); (h) at B = 4096; the index build with the exact dep_cap found by a first refused build (the wrapper's default guess fits both vocabularies).")
    emit()
    emit("summary")
    for s in summary:
        emit("  " + s)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
