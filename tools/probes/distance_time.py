"""window_join / distance at 1M x 1M synth tables (profiles/r05a_distance_1Mx1M.json.log): host clock around calls
that end in a device synchronise, the variants alternating, median and spread of 15 repeats after 3 warm-ups; per-phase
times from one profiled call each; the distance kernel on the N = 1000 pairs.  Run from the repository root:

    PYTHONPATH=. python tools/probes/distance_time.py
"""
import json, statistics, sys, time
import numpy as np, torch
from giql_amd import synth
from giql_amd.engine import DeviceSide, HipEngine

out = {}
eng = HipEngine(0)
ac, as_, ae = synth.make_table(1_000_000, 21, "peaks")
bc, bs, be = synth.make_table(1_000_000, 22, "peaks")
a, b = DeviceSide.from_numpy(ac, as_, ae), DeviceSide.from_numpy(bc, bs, be)

def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r

def plan_fill_inner():
    n = eng.inner_plan(a, b, 24)
    ra = torch.empty(n, dtype=torch.int32, device=eng.device); rb = torch.empty_like(ra)
    eng.inner_fill(ra, rb)
    return ra, rb

variants = {"inner_join (one call)": lambda: eng.inner_join(a, b, 24),
            "inner plan + fill": plan_fill_inner,
            "window_join N=0": lambda: eng.window_join(a, b, 24, 0),
            "window_join N=1000": lambda: eng.window_join(a, b, 24, 1000)}
times = {k: [] for k in variants}
pairs = {}
for rep in range(18):
    for k, fn in variants.items():
        ms, r = timed(fn)
        if rep >= 3:
            times[k].append(ms)
        pairs[k] = int(r[0].shape[0])
        st = eng.stats()
        if rep == 17:
            out.setdefault("forms", {})[k] = {kk: st[kk] for kk in ("join_form", "sort_local", "count_fused", "bucket_join", "fused_fill", "span_hist", "swapped")}
        del r
for k, v in times.items():
    out[k] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "pairs": pairs[k]}
assert pairs["window_join N=0"] == pairs["inner_join (one call)"] == pairs["inner plan + fill"]
# same multiset at N = 0 (order-independent check on the device: sorted packed pairs)
ra, rb = eng.window_join(a, b, 24, 0); ia, ib = eng.inner_join(a, b, 24)
pk = lambda x, y: torch.sort(x.long() * (1 << 32) + y.long()).values
assert torch.equal(pk(ra, rb), pk(ia, ib))
out["n0_same_multiset"] = True
# phases of one profiled window_join
eng.set_profiling(True)
for n in (0, 1000):
    eng.window_join(a, b, 24, n); torch.cuda.synchronize()
    st = eng.stats()
    out[f"phase_ms N={n}"] = {k: round(v, 4) for k, v in st["phase_ms"].items() if v > 0}
eng.inner_plan(a, b, 24); torch.cuda.synchronize()
out["phase_ms inner plan"] = {k: round(v, 4) for k, v in eng.stats()["phase_ms"].items() if v > 0}
eng.set_profiling(False)
# the distance kernel on the N = 1000 pairs
ra, rb = eng.window_join(a, b, 24, 1000)
n = int(ra.shape[0])
ts = []
for rep in range(23):
    ms, r = timed(lambda: eng.distance(a, b, ra, rb))
    if rep >= 3:
        ts.append(ms)
eng.set_profiling("aux")
eng.distance(a, b, ra, rb); torch.cuda.synchronize()
k_ms = eng.stats()["phase_ms"]["aux"]
eng.set_profiling(False)
d, v = eng.distance(a, b, ra, rb)
assert int(v.sum()) == n and int(d.max()) <= 1000 and int(d.min()) == 0
out["distance"] = {"pairs": n, "call_median_ms": round(statistics.median(ts), 4), "call_min_ms": round(min(ts), 4),
                   "call_max_ms": round(max(ts), 4), "kernel_ms": round(k_ms, 4), "algorithmic_bytes": 33 * n,
                   "kernel_GBps": round(33 * n / (k_ms * 1e-3) / 1e9, 1), "share_of_8TBps": round(33 * n / (k_ms * 1e-3) / 8e12, 4)}
# sorted pairs (grouped by A row) for the same kernel: the gathers' locality
order = torch.argsort(ra.long() * (1 << 32) + rb.long())
sa_, sb_ = ra[order].contiguous(), rb[order].contiguous()
eng.set_profiling("aux")
eng.distance(a, b, sa_, sb_); torch.cuda.synchronize()
out["distance"]["kernel_ms_pairs_sorted_by_row"] = round(eng.stats()["phase_ms"]["aux"], 4)
print(json.dumps(out, indent=1))
