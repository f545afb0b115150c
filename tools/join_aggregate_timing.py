#!/usr/bin/env python3
"""Time the map query -- SUM + AVG + COUNT of a right-table column grouped by the left interval -- both ways.

Seeded ``synth`` tables (the headline's generator): 1M "peaks" rows against 10M "peaks" rows with a float64 ``score``
column (about a fifth of it NULL), 24 chromosomes.  The same query text runs through ``execute`` twice:

* ``join_aggregates=True``: the pairs stay on the device and are aggregated per left row there
  (``giql_hip_pair_agg_dev``), the host combines 1M per-row partials;
* flag off: the pairs' key and score columns are gathered per pair, brought to the host and grouped there by pyarrow
  (the LEFT form with ``outer_joins=True``).

Each way: ``--warmup`` runs, then ``--reps`` timed runs, ALTERNATING between the two ways so both see the same
machine; every run device-synchronised and timed on the host clock around the whole ``execute`` call (uploads of
the cached tables excluded by the warm-up, the result table on the host included).  Reports the median and the
spread (min, max) of each and whether the new median lies below the old path's whole spread; the two result tables
are compared.  Prints one JSON line per form and a summary line; needs a GPU.

    python tools/join_aggregate_timing.py [--rows-a 1000000] [--rows-b 10000000] [--reps 5] [--warmup 1]
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

IV = "a.chrom, a.start, a.end"
QUERY = ("SELECT {iv}, SUM(b.score) AS total, AVG(b.score) AS mean, COUNT({count}) AS n "
         "FROM a {join} JOIN b ON a.interval INTERSECTS b.interval GROUP BY {iv}")
#: form -> (query, the other opt-ins of the flag-off run).  The LEFT form counts rows (COUNT(*)): a COUNT(b.col)
#: beside other aggregates does not lower without the flag.
FORMS = {
    "inner": (QUERY.format(iv=IV, join="INNER", count="b.score"), {}),
    "left": (QUERY.format(iv=IV, join="LEFT", count="*"), {"outer_joins": True}),
}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-a", type=int, default=1_000_000)
    ap.add_argument("--rows-b", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=20250)
    args = ap.parse_args()

    import pyarrow as pa
    import torch

    from giql_amd import synth
    from giql_amd.engine import HipEngine
    from giql_amd.execute import execute

    if not torch.cuda.is_available():
        print("join_aggregate_timing: no GPU", file=sys.stderr)
        return 2
    eng = HipEngine(0)

    def table(n, seed, score):
        c, s, e = synth.make_table(n, seed, "peaks")
        cols = {"chrom": pa.array(c, pa.int32()), "start": pa.array(s, pa.int32()), "end": pa.array(e, pa.int32())}
        if score:
            r = np.random.default_rng(seed + 7)
            cols["score"] = pa.array(r.normal(0, 100, n), mask=r.random(n) < 0.2)
        return pa.table(cols)

    tables = {"a": table(args.rows_a, args.seed + 1, False), "b": table(args.rows_b, args.seed + 3, True)}

    def timed(query, **opts):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = execute(query, tables, eng, giql_tables=["a", "b"], **opts)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def spread(ms):
        x = np.sort(np.asarray(ms))
        return {"median_ms": round(float(np.median(x)), 3), "min_ms": round(float(x[0]), 3),
                "max_ms": round(float(x[-1]), 3), "reps": int(x.size)}

    def same(new, old):
        keys = [(k, "ascending") for k in ("chrom", "start", "end")]
        new, old = new.sort_by(keys), old.sort_by(keys)
        if new.column_names != old.column_names or new.num_rows != old.num_rows:
            return False
        for name in new.column_names:
            x, y = new.column(name), old.column(name)
            if pa.types.is_floating(x.type):   # two summation orders: equal to a relative 1e-9 of the magnitudes summed
                xv, yv = (np.nan_to_num(v.to_numpy(zero_copy_only=False).astype(np.float64)) for v in (x, y))
                if x.null_count != y.null_count or not np.allclose(xv, yv, rtol=1e-9, atol=1e-6):
                    return False
            elif not x.equals(y):
                return False
        return True

    # the stage alone: giql_hip_pair_agg_dev over the join's own pairs (a float SUM: both sorts run)
    ra, rb = execute(FORMS["inner"][0], tables, eng, giql_tables=["a", "b"], return_indices=True)
    ra, rb = (torch.from_numpy(np.ascontiguousarray(x)).to(eng.device) for x in (ra, rb))
    score = tables["b"].column("score").combine_chunks()
    vals = torch.from_numpy(score.fill_null(0).to_numpy(zero_copy_only=False)).to(eng.device)
    valid = torch.from_numpy(score.is_valid().to_numpy(zero_copy_only=False).astype(np.uint8)).to(eng.device)
    aggs = [("SUM", vals, valid), ("AVG", vals, valid), ("COUNT", None, valid)]
    stage = []
    for k in range(args.warmup + args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.pair_aggregate(ra, rb, args.rows_a, args.rows_b, aggs)
        torch.cuda.synchronize()
        if k >= args.warmup:
            stage.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"stage": "pair_aggregate", "pairs": int(ra.shape[0]), "rows_a": args.rows_a,
                      "rows_b": args.rows_b, **spread(stage)}), flush=True)
    del ra, rb, vals, valid

    summary = []
    for form, (query, old_opts) in FORMS.items():
        for _ in range(max(args.warmup, 1)):
            _ms, new = timed(query, join_aggregates=True, **old_opts)
            _ms, old = timed(query, **old_opts)
        equal = same(new, old)
        t_new, t_old = [], []
        for _ in range(args.reps):
            t_new.append(timed(query, join_aggregates=True, **old_opts)[0])
            t_old.append(timed(query, **old_opts)[0])
        sn, so = spread(t_new), spread(t_old)
        faster = sn["median_ms"] < so["min_ms"]
        slower = sn["min_ms"] > so["median_ms"] and sn["median_ms"] > so["max_ms"]
        rec = {"form": form, "rows_a": args.rows_a, "rows_b": args.rows_b, "groups": new.num_rows,
               "outputs_equal": bool(equal), "join_aggregates": sn, "flag_off": so,
               "ratio": round(so["median_ms"] / sn["median_ms"], 3), "new_faster": bool(faster), "new_slower": bool(slower)}
        print(json.dumps(rec), flush=True)
        summary.append(rec)
    ok = all(r["outputs_equal"] for r in summary)
    print(json.dumps({"summary": [{"form": r["form"], "ratio": r["ratio"], "new_faster": r["new_faster"],
                                   "outputs_equal": r["outputs_equal"]} for r in summary], "all_outputs_equal": ok}),
          flush=True)
    eng.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
