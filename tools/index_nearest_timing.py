#!/usr/bin/env python3
"""Time NEAREST (k = 1) against a table index beside the ordinary operator.

Seeded ``synth`` tables on one context: "peaks" query tables (default 1M and 10M rows) against a fixed-length
("reads") and a general ("peaks") indexed table (default 10M rows), 24 chromosomes.  For each form and size the
ordinary call (``HipEngine.nearest``: ``giql_hip_nearest_dev``) and the indexed call (``HipEngine.nearest_indexed``:
``giql_hip_nearest_indexed_dev``) ALTERNATE in one process, after a warm-up of both, every repetition
device-synchronised; the median and the spread (min, max, quartiles) of each are reported.  Before timing the outputs
are asserted equal: the distances, which rows have a target, and the chosen target's (start, end) -- the row id
itself may differ between targets that share (distance, start, end).  The index build time, the preparation time
and the index's size before and after the preparation are given beside them.

"faster" means: the indexed call's upper quartile lies below the ordinary call's whole spread (its minimum).  A form
is routed by ``execute()`` only when it is faster at every size (``routed_by_rule`` of the summary line).

Prints one JSON line per measurement and a summary line; needs a GPU.

    python tools/index_nearest_timing.py [--rows-b 10000000] [--rows-a 1000000,10000000] [--reps 30] [--warmup 5]
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-b", type=int, default=10_000_000)
    ap.add_argument("--rows-a", default="1000000,10000000")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20251)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    sizes = [int(x) for x in args.rows_a.split(",")]

    import torch

    from giql_amd import synth
    from giql_amd.engine import DeviceSide, HipEngine

    if not torch.cuda.is_available():
        print("index_nearest_timing: no GPU", file=sys.stderr)
        return 2
    eng = HipEngine(0)
    enc = ("0based", "half_open")

    def side(n, seed, kind):
        c, s, e = synth.make_table(n, seed, kind)
        return DeviceSide.from_numpy(c, s, e, enc, device=eng.device)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def spread(ms):
        x = np.sort(np.asarray(ms))
        q1, q3 = np.percentile(x, [25, 75])
        return {"median_ms": round(float(np.median(x)), 4), "min_ms": round(float(x[0]), 4),
                "max_ms": round(float(x[-1]), 4), "q1_ms": round(float(q1), 4), "q3_ms": round(float(q3), 4),
                "reps": int(x.size)}

    def equal(want, got, b):
        (wi, wd), (gi, gd) = want, got
        if not (torch.equal(wd, gd) and torch.equal(wi >= 0, gi >= 0)):
            return False
        m = wi >= 0
        w, g = wi[m].long(), gi[m].long()
        return bool(torch.equal(b.start[w], b.start[g]) and torch.equal(b.end[w], b.end[g]))

    queries = [side(n, args.seed + 1 + k, "peaks") for k, n in enumerate(sizes)]
    summary = []
    for form, kind_b in (("fixed_length", "reads"), ("general", "peaks")):
        b = side(args.rows_b, args.seed + (20 if kind_b == "reads" else 30), kind_b)
        build_ms, index = timed(lambda: eng.index_create(b, 24))
        bytes_created = index.nbytes
        prepare_ms, _ = timed(index.prepare_nearest)
        print(json.dumps({"form": form, "rows_b": b.n, "index_general": index.general,
                          "index_build_ms": round(build_ms, 3), "prepare_nearest_ms": round(prepare_ms, 3),
                          "index_bytes_created": bytes_created, "index_bytes_prepared": index.nbytes}), flush=True)
        for a in queries:
            for signed in (False, True):
                want = eng.nearest(a, b, 24, signed=signed)
                got = eng.nearest_indexed(a, index, signed=signed)
                torch.cuda.synchronize()
                assert equal(want, got, b), (form, a.n, signed)
            ordinary = lambda: eng.nearest(a, b, 24)                 # noqa: E731
            indexed = lambda: eng.nearest_indexed(a, index)          # noqa: E731
            for _ in range(args.warmup):
                ordinary(), indexed()
            t_ord, t_idx = [], []
            for _ in range(args.reps):           # alternating: both see the same machine
                t_ord.append(timed(ordinary)[0])
                t_idx.append(timed(indexed)[0])
            so, si = spread(t_ord), spread(t_idx)
            faster = si["q3_ms"] < so["min_ms"]
            print(json.dumps({"form": form, "op": "NEAREST", "rows_a": a.n, "rows_b": b.n, "outputs_equal": True,
                              "ordinary": so, "indexed": si, "ratio": round(so["median_ms"] / si["median_ms"], 3),
                              "indexed_faster": bool(faster)}), flush=True)
            summary.append((form, a.n, bool(faster)))
        index.close()
        del b
    routed = {form: all(fa for f, _n, fa in summary if f == form) for form in ("fixed_length", "general")}
    print(json.dumps({"summary": [{"form": f, "rows_a": n, "indexed_faster": fa} for f, n, fa in summary],
                      "routed_by_rule": routed}), flush=True)
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
