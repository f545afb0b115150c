#!/usr/bin/env python3
"""Time COUNT / SEMI / ANTI against a table index beside the ordinary operators.

Seeded ``synth`` tables: a query table (default 1M "peaks" rows) against a fixed-length ("reads") and a general
("peaks") indexed table (default 10M rows), 24 chromosomes.  For each form and operator the ordinary call
(``giql_hip_count_dev`` / ``giql_hip_semi_anti_dev``) and the indexed call (``giql_hip_count_indexed_dev`` /
``giql_hip_semi_anti_indexed_dev``) ALTERNATE in one process, after a warm-up of both, every repetition
device-synchronised; the median and the spread (min, max, inter-quartile range) of each are reported, the outputs
are compared, and the index build and prepare times are given beside them.  "faster" means: the indexed median lies
below the ordinary call's whole spread (its minimum).

Prints one JSON line per measurement and a summary line; needs a GPU.

    python tools/index_rows_timing.py [--rows-b 10000000] [--rows-a 1000000] [--reps 30] [--warmup 5]
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
    ap.add_argument("--rows-a", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20250)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")

    import torch

    from giql_amd import synth
    from giql_amd.engine import DeviceSide, HipEngine

    if not torch.cuda.is_available():
        print("index_rows_timing: no GPU", file=sys.stderr)
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
                "max_ms": round(float(x[-1]), 4), "iqr_ms": round(float(q3 - q1), 4), "reps": int(x.size)}

    a = side(args.rows_a, args.seed + 1, "peaks")
    summary = []
    for form, kind_b in (("fixed_length", "reads"), ("general", "peaks")):
        b = side(args.rows_b, args.seed + (2 if kind_b == "reads" else 3), kind_b)
        build_ms, index = timed(lambda: eng.index_create(b, 24))
        prepare_ms, _ = timed(index.prepare_rows)
        print(json.dumps({"form": form, "rows_b": b.n, "rows_a": a.n, "index_general": index.general,
                          "index_build_ms": round(build_ms, 3), "prepare_rows_ms": round(prepare_ms, 3),
                          "index_bytes": index.nbytes}), flush=True)
        ops = {
            "COUNT": (lambda: eng.count_overlaps(a, b, 24), lambda: eng.count_overlaps_indexed(a, index)),
            "SEMI": (lambda: eng.semi_anti(a, b, 24, False), lambda: eng.semi_anti_indexed(a, index, False)),
            "ANTI": (lambda: eng.semi_anti(a, b, 24, True), lambda: eng.semi_anti_indexed(a, index, True)),
        }
        for op, (ordinary, indexed) in ops.items():
            for _ in range(args.warmup):
                want, got = ordinary(), indexed()
            torch.cuda.synchronize()
            equal = bool(torch.equal(want, got))
            t_ord, t_idx = [], []
            for _ in range(args.reps):           # alternating: both see the same machine
                t_ord.append(timed(ordinary)[0])
                t_idx.append(timed(indexed)[0])
            so, si = spread(t_ord), spread(t_idx)
            faster = si["median_ms"] < so["min_ms"]
            rec = {"form": form, "op": op, "rows_a": a.n, "rows_b": b.n, "outputs_equal": equal, "n_out": int(got.shape[0]),
                   "ordinary": so, "indexed": si, "ratio": round(so["median_ms"] / si["median_ms"], 3),
                   "indexed_faster": bool(faster)}
            print(json.dumps(rec), flush=True)
            summary.append((form, op, equal, faster))
        index.close()
        del b
    ok = all(eq for _f, _o, eq, _fa in summary)
    print(json.dumps({"summary": [{"form": f, "op": o, "outputs_equal": eq, "indexed_faster": fa}
                                  for f, o, eq, fa in summary], "all_outputs_equal": ok}), flush=True)
    eng.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
