#!/usr/bin/env python3
"""Time the disjoint-partition recipe -- SELECT DISTINCT disjoin_chrom, disjoin_start, disjoin_end FROM DISJOIN(t) --
both ways.

The query exists with and without ``disjoin_aggregates``:

* flag on: the segments come straight from the breakpoint table (``giql_hip_coverage_dev``), at most 2n - 1 rows;
* flag off: DISJOIN writes one row per (parent, piece), ``execute`` brings them to the host and deduplicates there.

Seeded ``synth`` tables, 24 chromosomes: a sparse one ("peaks", 10M rows, mean depth about 3.5) and a deep one -- the
same generator, every row lengthened about its start until the mean depth is near ``--depth`` (30), with few enough
rows that the flag-off piece count (printed) fits one card.  Each way: ``--warmup`` runs, then ``--reps`` timed runs,
ALTERNATING between the two ways so both see the same machine; every run device-synchronised and timed on the host
clock around the whole ``execute`` call (uploads of the cached tables excluded by the warm-up, the result table on the
host included).  Reports the median and the spread (min, max) of each and whether the new median lies below the
flag-off path's whole spread; the two result tables are compared as row sets.  Prints one JSON line per table and a
summary line; needs a GPU.

    python tools/coverage_timing.py [--rows-sparse 10000000] [--rows-deep 500000] [--depth 30] [--reps 5] [--warmup 1]
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

QUERY = "SELECT DISTINCT disjoin_chrom, disjoin_start, disjoin_end FROM DISJOIN(features)"


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-sparse", type=int, default=10_000_000)
    ap.add_argument("--rows-deep", type=int, default=500_000)
    ap.add_argument("--depth", type=float, default=30.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=20260)
    args = ap.parse_args()

    import pyarrow as pa
    import torch

    from giql_amd import synth
    from giql_amd.engine import HipEngine
    from giql_amd.execute import clear_caches, execute

    if not torch.cuda.is_available():
        print("coverage_timing: no GPU", file=sys.stderr)
        return 2
    eng = HipEngine(0)
    genome = float(synth.HG38_LENGTHS.sum())

    def table(n, seed, depth=None):
        c, s, e = synth.make_table(n, seed, "peaks")
        if depth is not None:   # the same rows, lengthened about their start to the asked mean depth
            ln = (e - s).astype(np.int64)
            factor = depth * genome / float(ln.sum())
            e = np.minimum(s.astype(np.int64) + np.round(ln * factor).astype(np.int64),
                           synth.HG38_LENGTHS[c]).astype(np.int32)
        mean_depth = float((e.astype(np.int64) - s).sum()) / genome
        return pa.table({"chrom": pa.array(c, pa.int32()), "start": pa.array(s, pa.int32()),
                         "end": pa.array(e, pa.int32())}), mean_depth

    def spread(ms):
        x = np.sort(np.asarray(ms))
        return {"median_ms": round(float(np.median(x)), 3), "min_ms": round(float(x[0]), 3),
                "max_ms": round(float(x[-1]), 3), "reps": int(x.size)}

    def same(new, old):
        keys = [(k, "ascending") for k in ("disjoin_chrom", "disjoin_start", "disjoin_end")]
        if new.column_names != old.column_names or new.num_rows != old.num_rows:
            return False
        new, old = new.sort_by(keys), old.sort_by(keys)
        return all(np.array_equal(new.column(k).to_numpy(), old.column(k).to_numpy()) for k in new.column_names)

    summary = []
    for name, rows, depth in (("sparse", args.rows_sparse, None), ("deep", args.rows_deep, args.depth)):
        tbl, mean_depth = table(rows, args.seed + (1 if depth is None else 3), depth)
        tables = {"features": tbl}

        def timed(**opts):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = execute(QUERY, tables, eng, giql_tables=["features"], **opts)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, out

        pieces = int(execute("SELECT disjoin_start FROM DISJOIN(features)", tables, eng, giql_tables=["features"],
                             return_indices=True)[0].shape[0])
        print(json.dumps({"table": name, "rows": rows, "mean_depth": round(mean_depth, 2), "flag_off_pieces": pieces}),
              file=sys.stderr, flush=True)
        for _ in range(max(args.warmup, 1)):
            _ms, new = timed(disjoin_aggregates=True)
            _ms, old = timed()
        equal = same(new, old)
        segments = new.num_rows
        del new, old
        t_new, t_old = [], []
        for k in range(args.reps):
            t_new.append(timed(disjoin_aggregates=True)[0])
            t_old.append(timed()[0])
            print(f"  {name} rep {k}: {t_new[-1]:.1f} ms against {t_old[-1]:.1f} ms", file=sys.stderr, flush=True)
        sn, so = spread(t_new), spread(t_old)
        rec = {"table": name, "rows": rows, "mean_depth": round(mean_depth, 2), "flag_off_pieces": pieces,
               "segments": segments, "outputs_equal": bool(equal), "disjoin_aggregates": sn, "flag_off": so,
               "ratio": round(so["median_ms"] / sn["median_ms"], 3),
               "new_faster": bool(sn["median_ms"] < so["min_ms"]),
               "new_slower": bool(sn["min_ms"] > so["median_ms"] and sn["median_ms"] > so["max_ms"])}
        print(json.dumps(rec), flush=True)
        summary.append(rec)
        del tables, tbl
        clear_caches()
    ok = all(r["outputs_equal"] for r in summary)
    print(json.dumps({"summary": [{"table": r["table"], "ratio": r["ratio"], "new_faster": r["new_faster"],
                                   "outputs_equal": r["outputs_equal"]} for r in summary], "all_outputs_equal": ok}),
          flush=True)
    eng.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
