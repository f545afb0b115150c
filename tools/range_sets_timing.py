#!/usr/bin/env python3
"""Time ``interval INTERSECTS ANY(K ranges)`` as a filter (``HipEngine.range_set_any`` + select) beside the route a
user had before it for the same answer: the K ranges loaded into a table and a SEMI JOIN against it.

Seeded ``synth`` tables of fixed-length "reads" over 24 chromosomes; K seeded ranges of 1-20 kb spread over the same
chromosomes.  Per (rows, K), ALTERNATING in one process after a warm-up of all four, every repetition
device-synchronised:

  (a) ``set_call``      ``HipEngine.range_set_any`` on the device-resident columns (host preparation of the set, its
                        upload, the kernel, the synchronise);
  (b) ``semi_call``     ``HipEngine.semi_anti`` of the table against the K ranges as a device-resident side;
  (c) ``set_execute``   ``execute("... WHERE interval INTERSECTS ANY(...)", range_sets=True, return_indices=True)`` on
                        the pinned Arrow table (device copy and codes reused): plan, kernel, select, ids to the host;
  (d) ``semi_execute``  ``execute("SELECT a.start FROM t a SEMI JOIN ranges b ON a.interval INTERSECTS b.interval", return_indices=True)``
                        on the same pinned table.

The row ids of (c) and (d) are compared first.  The kernel's own time is taken in a separate pass with the context's
profiling on (device events around the launch: ``stats()["phase_ms"]["aux"]``), as is the SEMI call's device time
(``total_ms``); the kernel's read rate is the 12 bytes per row it must read over that time, beside the device's
single-array read rate measured in the same process (``HipEngine.stream_probe``).  Reported per quantity: median, min,
max, inter-quartile range; and whether the set route's median lies below the SEMI route's whole spread.  Prints one
JSON line per (rows, K) and a summary line; needs a GPU.

    python tools/range_sets_timing.py [--rows 10000000,100000000] [--k 2,64,1024] [--reps 7] [--warmup 2]
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
    ap.add_argument("--rows", default="10000000,100000000")
    ap.add_argument("--k", default="2,64,1024")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-probe", action="store_true", help="skip the stream probe (the read-rate ceiling)")
    args = ap.parse_args()

    import pyarrow as pa
    import torch

    import giql_amd
    from giql_amd import synth
    from giql_amd.engine import DeviceSide, HipEngine
    from giql_amd.execute import execute

    if not torch.cuda.is_available():
        print("range_sets_timing: no GPU", file=sys.stderr)
        return 2
    eng = HipEngine(0)
    prof = HipEngine(0, profiling=True)
    names = synth.HG38_NAMES

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

    read_gbps = None
    if not args.no_probe:
        read_gbps = eng.stream_probe(shapes=[(4, 1, 8), (8, 1, 8), (8, 1, 16)])["read"]
    summary = []
    for n in (int(x) for x in args.rows.split(",")):
        chrom, start, end = synth.make_table(n, 4242, "reads")
        side = DeviceSide.from_numpy(chrom, start, end, device=eng.device)
        table = pa.table({"chrom": pa.DictionaryArray.from_arrays(pa.array(chrom, pa.int32()), pa.array(names)),
                          "start": pa.array(start), "end": pa.array(end)})
        pinned = giql_amd.pin(table)
        for k in (int(x) for x in args.k.split(",")):
            r = np.random.default_rng(k)
            rc = r.integers(0, len(names), k).astype(np.int32)
            lo = (r.random(k) * (synth.HG38_LENGTHS[rc] - 30_000)).astype(np.int64)
            hi = lo + r.integers(1_000, 20_000, k)
            ranges_side = DeviceSide.from_numpy(rc, lo.astype(np.int32), hi.astype(np.int32), device=eng.device)
            ranges_table = pa.table({"chrom": pa.array([names[c] for c in rc]), "start": pa.array(lo.astype(np.int32)),
                                     "end": pa.array(hi.astype(np.int32))})
            literals = ", ".join(f"'{names[c]}:{a}-{b}'" for c, a, b in zip(rc, lo, hi))
            q_set = f"SELECT * FROM t WHERE interval INTERSECTS ANY({literals})"
            q_semi = "SELECT a.start FROM t a SEMI JOIN ranges b ON a.interval INTERSECTS b.interval"
            one_set = [("intersects", rc, hi, lo)]
            runs = {
                "set_call": lambda: eng.range_set_any(side.chrom, side.start, side.end, one_set),
                "semi_call": lambda: eng.semi_anti(side, ranges_side, len(names), False),
                "set_execute": lambda: execute(q_set, {"t": pinned}, eng, return_indices=True, range_sets=True),
                "semi_execute": lambda: execute(q_semi, {"t": pinned, "ranges": ranges_table}, eng,
                                                         return_indices=True),
            }
            ids_set, ids_semi = runs["set_execute"](), runs["semi_execute"]()
            same = bool(np.array_equal(np.sort(ids_set), np.sort(ids_semi)))
            ms = {name: [] for name in runs}
            for rep in range(args.warmup + args.reps):
                for name, fn in runs.items():
                    t, _ = timed(fn)
                    if rep >= args.warmup:
                        ms[name].append(t)
            # device time, profiling on, in a pass of its own
            kernel_ms, semi_dev_ms = [], []
            for rep in range(args.warmup + args.reps):
                prof.range_set_any(side.chrom, side.start, side.end, one_set)
                a = prof.stats()["phase_ms"]["aux"]
                prof.semi_anti(side, ranges_side, len(names), False)
                b = prof.stats()["total_ms"]
                if rep >= args.warmup:
                    kernel_ms.append(a)
                    semi_dev_ms.append(b)
            line = {"rows": n, "k": k, "kept": int(ids_set.size), "same_ids": same,
                    **{name: spread(v) for name, v in ms.items()},
                    "set_kernel": spread(kernel_ms), "semi_device": spread(semi_dev_ms)}
            km = line["set_kernel"]["median_ms"]
            line["set_kernel_read_GBps"] = round(12.0 * n / (km * 1e-3) / 1e9, 1) if km > 0 else None
            line["measured_read_GBps"] = read_gbps
            line["set_call_wins"] = line["set_call"]["median_ms"] < line["semi_call"]["min_ms"]
            line["set_execute_wins"] = line["set_execute"]["median_ms"] < line["semi_execute"]["min_ms"]
            print(json.dumps(line), flush=True)
            summary.append((n, k, same, line["set_call_wins"], line["set_execute_wins"]))
        pinned.unpin()
        del side, table, pinned
        giql_amd.clear_caches()
    print(json.dumps({"summary": [{"rows": n, "k": k, "same_ids": s, "set_call_wins": a, "set_execute_wins": b}
                                  for n, k, s, a, b in summary]}), flush=True)
    return 0 if all(s for _n, _k, s, _a, _b in summary) else 1


if __name__ == "__main__":
    sys.exit(main())
