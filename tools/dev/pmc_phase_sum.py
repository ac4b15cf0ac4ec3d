"""Per-phase counter sums of a tools/dev/gpu_phase_mix.py run under rocprofv3 --pmc (python tools/dev/pmc_phase_sum.py RESULTS.db): k_pretok's dispatches in order, WARM skipped, then groups of N for stops 0 7 6 5 4 3 2 1."""
import sqlite3, sys
from collections import defaultdict
WARM, N = 30, 20
db = sqlite3.connect(sys.argv[1])
cols = [r[1] for r in db.execute("pragma table_info(pmc_events)")]
cname = "counter_name" if "counter_name" in cols else "pmc_name"
vname = "counter_value" if "counter_value" in cols else "value"
per = defaultdict(dict)
for name, cn, val, did in db.execute(f"select name, {cname}, {vname}, dispatch_id from pmc_events"):
    if "k_pretok" in name:
        per[did][cn] = per[did].get(cn, 0.0) + val
ids = sorted(per)
print("k_pretok dispatches:", len(ids))
ids = ids[WARM:]
stops = (0, 7, 6, 5, 4, 3, 2, 1)
cum = {}
for gi, stop in enumerate(stops):
    g = ids[gi * N:(gi + 1) * N]
    cum[stop] = {c: sum(per[d].get(c, 0.0) for d in g) / max(len(g), 1) for c in sorted(per[ids[0]])}
ctrs = sorted(cum[0])
names = {1: "stage", 2: "classify + masks", 3: "starts", 4: "chunk list", 5: "(5 = 4)", 6: "probe", 7: "merge", 0: "tail + tile record + hand-over"}
print(f"{'up to / phase':34s}" + "".join(f"{c:>20s}" for c in ctrs))
prev = {c: 0.0 for c in ctrs}
for stop in (1, 2, 3, 4, 5, 6, 7, 0):
    print(f"cumulative, stop {stop:<15d}" + " " * 8 + "".join(f"{cum[stop][c]:20.0f}" for c in ctrs))
prev = {c: 0.0 for c in ctrs}
for stop in (1, 2, 3, 4, 5, 6, 7, 0):
    print(f"phase  {names[stop]:27s}" + "".join(f"{cum[stop][c] - prev[c]:20.0f}" for c in ctrs))
    prev = cum[stop]
