"""Draft verification on the GPU against what a caller can do without it -> profiles/draft_mask.txt.

  (d) the draft call       spl_dfa_draft_device / spl_nest_draft_device: ONE launch, masks [B, 1 + K, n_words], ok, live and the states
  (r) the reference route  a chain: K + 1 calls of spl_dfa_step_device / spl_nest_step_device with lengths 0 .. K into scratch states and the
                           slices of a mask [1 + K, B, n_words]; the tree: one step call per node with its path (the paths gathered BEFORE
                           the clock starts: that favours the reference).  MEASURED IN THE SAME RUN, twice, so that its own two medians say
                           what a difference means
  (w) the guides           RegexGuide.draft / NestGuide.draft, wall time, outputs allocated inside

cl100k_base and o200k_base; B = 16, 64, 256; a chain of K = 4 and 8 and a 26-node static tree (TREE below, EAGLE style: wide at the root,
five deep); the regex guide on tools/dfa_bench.py's JSON shape, json_table() at tools/nest_bench.py's value boundaries (v): every draft id
is acceptable (a node at depth d carries the d-th id of a script), so every row is a constrained row with its dependent ids walked.
Device events around bursts of 16 calls.  No number here is a bar: none existed."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from choice_bench import vocabulary  # noqa: E402
from dfa_bench import STEP_PATTERN, lowest_allowed  # noqa: E402
from stream_bench import stat  # noqa: E402
from splintr_amd import Tokenizer, _ffi, dfa, nest  # noqa: E402
from splintr_amd import device as dv  # noqa: E402

CALLS, WARM, ROUNDS = 16, 3, 15
TREE = [-1, -1, -1, -1, 0, 0, 0, 1, 1, 2, 4, 4, 5, 7, 10, 10, 11, 14, 14, 17, 3, 8, 12, 15, 18, 19]
DEPTH = 4


def paths_of(parent):
    out = []
    for i, p in enumerate(parent):
        out.append((out[p] if p >= 0 else []) + [i])
    return out


def event_bursts(contenders):
    """{name: [ms per call, one per burst]}: every burst is CALLS calls between two device events, nothing copied to the host"""
    import time
    out = {name: [] for name in contenders}
    wall = {name: [] for name in contenders}
    for r in range(WARM + ROUNDS):
        for name, call in contenders.items():
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            for _ in range(CALLS):
                call()
            b.record()
            torch.cuda.synchronize()
            if r >= WARM:
                out[name].append(a.elapsed_time(b) / CALLS)
                wall[name].append((time.perf_counter() - t0) * 1e3 / CALLS)
    return out, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--vocabs", default="cl100k_base,o200k_base")
    ap.add_argument("--sizes", default="16,64,256")
    args = ap.parse_args()
    if not torch.cuda.is_available() or _ffi.lib().spl_device_count() == 0:
        sys.exit("draft_bench: no GPU")
    dev = torch.device("cuda", 0)
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    emit(f"draft_bench: {torch.cuda.get_device_name(0)}; library {os.path.basename(_ffi.LIB_PATH)}; bursts of {CALLS} calls, {ROUNDS} bursts; us per CALL "
         f"(device events; the guides: wall)")
    emit(f"the tree, {len(TREE)} nodes, parent row: {TREE}")
    summary, slower = [], []
    t_json = nest.json_table()
    d_shape = dfa.compile_regex(STEP_PATTERN)
    shapes = [("chain K=4", None, 4), ("chain K=8", None, 8), ("tree 26", TREE, len(TREE))]
    for name in args.vocabs.split(","):
        tok = Tokenizer.from_pretrained(name)
        toks, special = vocabulary(tok)
        one = {b: i for i, b in toks if len(b) == 1}
        nw = dv.dfa_n_words(tok)
        emit()
        emit(f"== {name}: V = {tok.vocab_size}, n_words = {nw}, END id {special}")
        for B in map(int, args.sizes.split(",")):
            rx = dv.RegexGuide(tok, B, d_shape, end_ids=[special])
            ng = dv.NestGuide(tok, B, t_json, end_ids=[special], max_depth=32)
            rx.begin()
            rx0 = rx.state.clone()
            script_rx = []
            for _ in range(8):
                ids = lowest_allowed(rx.mask).contiguous()
                script_rx.append(ids)
                rx.step(ids)
            assert rx.live.all().item()
            rx.state.copy_(rx0)
            ng.begin()
            for _ in range(DEPTH):
                ng.step(torch.full((B,), one[b"["], dtype=torch.int64, device=dev))
            script_ng = [torch.full((B,), one[b"1" if k % 2 == 0 else b","], dtype=torch.int64, device=dev) for k in range(8)]
            for label, parent, K in shapes:
                paths = paths_of(parent if parent is not None else [i - 1 for i in range(K)])
                t_par = None if parent is None else torch.tensor(parent, dtype=torch.int32, device=dev)
                for gname, g, script in (("regex guide, the JSON shape", rx, script_rx), ("json_table(), value boundaries", ng, script_ng)):
                    ids = torch.stack([script[len(p) - 1] for p in paths], dim=1).contiguous()
                    is_nest = g is ng
                    W = (5,) if is_nest else ()
                    mask = torch.empty((B, 1 + K, nw), dtype=torch.int32, device=dev)
                    r_mask = torch.empty((1 + K, B, nw), dtype=torch.int32, device=dev)
                    r_state = torch.empty((1 + K, B) + W, dtype=torch.int64, device=dev)
                    r_live = torch.empty((1 + K, B), dtype=torch.uint8, device=dev)
                    fed = [None] + [ids[:, p].contiguous() for p in paths]         # (gathered before the clock starts)
                    lens = [None] + [torch.full((B,), i + 1, dtype=torch.int32, device=dev) for i in range(K)]

                    def draft_call():
                        if is_nest:
                            return dv.nest_draft_device(tok, ids, None, g.state, g.table, g.index, n_states=g.n_states, n_ret=g.n_ret, dep_cap=g.n_dep,
                                                        end_ids=[special], max_depth=g.max_depth, parent=t_par, states=True, mask=mask)
                        return dv.dfa_draft_device(tok, ids, None, g.state, g.table, g.index, end_ids=[special], parent=t_par, n_states=g.n_states, states=True,
                                                   mask=mask)

                    def ref_call():
                        for r in range(1 + K):
                            x, n = (ids, lens[r]) if parent is None and r else (fed[r], None)
                            if is_nest:
                                dv.nest_step_device(tok, x, n, g.state, g.table, g.index, n_states=g.n_states, n_ret=g.n_ret, dep_cap=g.n_dep, end_ids=[special],
                                                    max_depth=g.max_depth, mask=r_mask[r], state_out=r_state[r], live=r_live[r])
                            else:
                                dv.dfa_step_device(tok, x, n, g.state, g.table, g.index, end_ids=[special], n_states=g.n_states, mask=r_mask[r],
                                                   state_out=r_state[r], live=r_live[r])
                    d = draft_call()
                    ref_call()
                    assert torch.equal(d.mask.transpose(0, 1), r_mask) and torch.equal(d.live.t(), r_live) and torch.equal(d.state.transpose(0, 1), r_state)
                    assert d.ok.all().item() and d.live.all().item(), "a draft id of the script was refused"
                    e, w = event_bursts({"d": draft_call, "r": ref_call, "r2": ref_call, "w": lambda: g.draft(ids, parent=t_par, states=True)})
                    md, mr, mr2, mw = (stat(e[k])[0] * 1e3 for k in ("d", "r", "r2", "w"))
                    ww = stat(w["w"])[0] * 1e3
                    gap = abs(mr - mr2)
                    verdict = "slower than both by more than their gap" if md > max(mr, mr2) + gap else "not slower"
                    emit(f"  {name} B={B:<4} {label:<10} {gname:<31} (d) {md:8.2f}  (r) {mr:8.2f} / {mr2:8.2f} (gap {gap:6.2f})  (w) guide.draft {mw:8.2f} dev, {ww:8.2f} wall"
                         f"   {(1 + K) * B * nw * 4 / 1e6:6.1f} MB of mask   (r)/(d) {min(mr, mr2) / md:5.2f}x   {verdict}")
                    summary.append(f"{name} B={B} {label} {gname}: draft {md:.1f} us, reference {mr:.1f} / {mr2:.1f} us, guide.draft wall {ww:.1f} us")
                    if md > max(mr, mr2) + gap:
                        slower.append(summary[-1])
    emit()
    emit("not measured: drafts with rejected ids (their rows are rows of ones: cheaper than these); a batch spread over many states' rows; per-sequence parents;")
    emit("the one-wavefront-per-sequence form (not built); the reference route with the paths gathered inside the clock.")
    emit()
    emit(f"shapes at which the draft call is slower than the reference route by more than the gap of the reference's own two medians: {len(slower)}")
    for s in slower:
        emit("  " + s)
    emit()
    emit("summary")
    for s in summary:
        emit("  " + s)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
