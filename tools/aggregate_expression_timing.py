#!/usr/bin/env python3
"""Time aggregates over an expression of a join's pair -- the "Overlap Statistics" query: COUNT(*), AVG and SUM of
``LEAST(a.end, b.end) - GREATEST(a.start, b.start)`` -- both ways, and the reduction stage on its own.

Seeded ``synth`` tables (the headline's generator): 1M "peaks" rows against 10M "peaks" rows with a float64 ``score``
column (about a fifth of it NULL), 24 chromosomes.  Two comparisons:

* the QUERY, grouped by the left interval and by ``a.chrom``: ``join_aggregates=True, aggregate_expressions=True``
  (the pairs stay on the device, the expression is evaluated inside the per-left-row reduction, the host combines 1M
  per-row partials) against the only route there was before: the ``select_expressions=True`` INNER query projecting
  the keys and the expression per pair, grouped on the host with pyarrow;
* the STAGE alone over the join's own pairs: ``pair_aggregate`` with ``("expr", tree)`` sources
  (``giql_hip_pair_expr_agg_dev``); the composition it replaces -- ``eval_exprs`` into a per-pair value array, then
  ``pair_aggregate(row_a, arange(n), n_a, n, ...)`` over that array; and ``giql_hip_pair_agg_dev`` with a column SUM
  on the same pairs, for what the interpreter costs on top of a gather.

Each way: ``--warmup`` runs, then ``--reps`` timed runs, ALTERNATING between the ways of a comparison so all see the
same machine; every run device-synchronised and timed on the host clock.  Reports the median and the spread (min,
max) of each; outputs are compared for equality (integers: exact).  Every step runs in a child process of its own
under its own time limit (``--step-timeout`` seconds); the first step that fails or runs out of time ends the run.
Prints one JSON line per measurement and a summary line; needs a GPU.

    python tools/aggregate_expression_timing.py [--rows-a 1000000] [--rows-b 10000000] [--reps 5] [--warmup 1]
"""

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OV = "LEAST(a.end, b.end) - GREATEST(a.start, b.start)"
KEYS = {"interval": "a.chrom, a.start, a.end", "chrom": "a.chrom"}
STEPS = ("stage", "query_interval", "query_chrom")


def spread(ms):
    x = np.sort(np.asarray(ms))
    return {"median_ms": round(float(np.median(x)), 3), "min_ms": round(float(x[0]), 3),
            "max_ms": round(float(x[-1]), 3), "reps": int(x.size)}


def run_step(args) -> int:
    import pyarrow as pa
    import torch

    from giql_amd import synth
    from giql_amd.engine import HipEngine
    from giql_amd.execute import execute

    if not torch.cuda.is_available():
        print("aggregate_expression_timing: no GPU", file=sys.stderr)
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

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def alternate(ways):
        """{name: callable} -> ({name: spread}, {name: last output}); warm-ups first, then the timed runs in turn."""
        times, outs = {k: [] for k in ways}, {}
        for rep in range(args.warmup + args.reps):
            for name, fn in ways.items():
                ms, outs[name] = clock(fn)
                if rep >= args.warmup:
                    times[name].append(ms)
        return {k: spread(v) for k, v in times.items()}, outs

    if args.step == "stage":
        ra, rb = execute("SELECT a.start FROM a JOIN b ON a.interval INTERSECTS b.interval", tables, eng,
                         giql_tables=["a", "b"], return_indices=True)
        ra, rb = (torch.from_numpy(np.ascontiguousarray(x)).to(eng.device) for x in (ra, rb))
        n = int(ra.shape[0])
        dev = {(t, c): torch.from_numpy(tables[t].column(c).to_numpy()).to(eng.device) for t in "ab" for c in ("start", "end")}
        tree = ("-", ("least", ("a", dev["a", "end"]), ("b", dev["b", "end"])),
                ("greatest", ("a", dev["a", "start"]), ("b", dev["b", "start"])))
        b_end = dev["b", "end"]
        ids = torch.arange(n, dtype=torch.int32, device=eng.device)

        def fused():
            return eng.pair_aggregate(ra, rb, args.rows_a, args.rows_b, [("SUM", ("expr", tree)), ("AVG", ("expr", tree))])

        def composed():
            vals, valid = eng.eval_exprs([tree], idx_a=ra, idx_b=rb, n_rows_a=args.rows_a, n_rows_b=args.rows_b)[0]
            return eng.pair_aggregate(ra, ids, args.rows_a, n, [("SUM", vals, valid), ("AVG", vals, valid)])

        def column():
            return eng.pair_aggregate(ra, rb, args.rows_a, args.rows_b, [("SUM", b_end, None), ("AVG", b_end, None)])

        times, outs = alternate({"fused": fused, "composed": composed, "column_sum": column})
        equal = all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
                    for x, y in zip(outs["fused"][1], outs["composed"][1])) and torch.equal(outs["fused"][0], outs["composed"][0])
        f, c = times["fused"], times["composed"]
        print(json.dumps({"stage": "pair_aggregate over an expression", "pairs": n, "rows_a": args.rows_a,
                          "rows_b": args.rows_b, **times, "outputs_equal": bool(equal),
                          "per_pair_value_bytes_avoided": 9 * n,
                          "fused_faster": bool(f["median_ms"] < c["min_ms"]),
                          "fused_slower": bool(f["min_ms"] > c["median_ms"] and f["median_ms"] > c["max_ms"])}), flush=True)
        return 0 if equal else 1

    kname = args.step[len("query_"):]
    keys = KEYS[kname]
    names = [k.split(".")[1] for k in keys.split(", ")]
    new_q = (f"SELECT {keys}, COUNT(*) AS overlap_count, AVG({OV}) AS avg_overlap_bp, SUM({OV}) AS total_overlap_bp "
             f"FROM a INNER JOIN b ON a.interval INTERSECTS b.interval GROUP BY {keys}")
    old_q = f"SELECT {keys}, {OV} AS overlap_bp FROM a INNER JOIN b ON a.interval INTERSECTS b.interval"

    def new():
        return execute(new_q, tables, eng, giql_tables=["a", "b"], join_aggregates=True, aggregate_expressions=True)

    def old():
        per_pair = execute(old_q, tables, eng, giql_tables=["a", "b"], select_expressions=True)
        g = per_pair.group_by(names, use_threads=False).aggregate([([], "count_all"), ("overlap_bp", "mean"), ("overlap_bp", "sum")])
        g = g.select(names + ["count_all", "overlap_bp_mean", "overlap_bp_sum"])
        return g.rename_columns(names + ["overlap_count", "avg_overlap_bp", "total_overlap_bp"])

    times, outs = alternate({"aggregate_expressions": new, "per_pair_then_host_group": old})
    order = [(k, "ascending") for k in names]
    x, y = outs["aggregate_expressions"].sort_by(order), outs["per_pair_then_host_group"].sort_by(order)
    equal = x.num_rows == y.num_rows and all(
        np.array_equal(x.column(c).to_numpy(), y.column(c).to_numpy()) if c != "avg_overlap_bp" else
        np.allclose(x.column(c).to_numpy(), y.column(c).to_numpy(), rtol=1e-12, atol=0.0) for c in x.column_names)
    sn, so = times["aggregate_expressions"], times["per_pair_then_host_group"]
    print(json.dumps({"query": "overlap statistics", "grouped_by": kname, "rows_a": args.rows_a, "rows_b": args.rows_b,
                      "groups": x.num_rows, "outputs_equal": bool(equal), **times,
                      "ratio": round(so["median_ms"] / sn["median_ms"], 3),
                      "new_faster": bool(sn["median_ms"] < so["min_ms"]),
                      "new_slower": bool(sn["min_ms"] > so["median_ms"] and sn["median_ms"] > so["max_ms"])}), flush=True)
    return 0 if equal else 1


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-a", type=int, default=1_000_000)
    ap.add_argument("--rows-b", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=20250)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds a step may take")
    ap.add_argument("--step", choices=STEPS, help="run this one step in this process (what the driver starts)")
    args = ap.parse_args()
    if args.step:
        return run_step(args)
    lines = []
    for step in STEPS:      # one child per step, each under its own time limit; nothing is started after a failure
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step,
               "--rows-a", str(args.rows_a), "--rows-b", str(args.rows_b), "--reps", str(args.reps),
               "--warmup", str(args.warmup), "--seed", str(args.seed)]
        done = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(done.stdout)
        sys.stdout.flush()
        if done.returncode != 0:
            sys.stderr.write(done.stderr[-4000:])
            print(json.dumps({"step": step, "failed_with": done.returncode}), flush=True)
            return 1
        lines += [json.loads(x) for x in done.stdout.splitlines() if x.startswith("{")]
    print(json.dumps({"summary": [{k: r[k] for k in ("stage", "query", "grouped_by", "ratio", "outputs_equal", "fused_faster",
                                                      "fused_slower", "new_faster", "new_slower") if k in r} for r in lines],
                      "all_outputs_equal": all(r["outputs_equal"] for r in lines)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
