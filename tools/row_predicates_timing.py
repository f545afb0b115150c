#!/usr/bin/env python3
"""Time SEMI / ANTI and COUNT over CONTAINS, WITHIN and DISTANCE <= N beside the same results composed from what
existed before them.

Seeded ``synth`` tables over 24 chromosomes, the two configurations of tools/left_join_timing.py: 1M "peaks" against
10M "reads", and the benchmark's own tables with the 100M-row one on the left (100M "reads" against 10M "peaks").
For each of the six forms -- {exists, count} x {contains, within, within_distance} -- two quantities, ALTERNATING in
one process after a warm-up of both, every repetition device-synchronised:

  (b) ``new``       ``HipEngine.semi_anti_pred`` (the SEMI call) / ``HipEngine.count_pred``;
  (c) ``composed``  the pair join (``contain_join`` / ``window_join``), then ``mark`` + ``select(flags = 1)`` for
                    SEMI, or ``torch.bincount`` of the left ids for COUNT.

The outputs of (b) and (c) are compared first (``torch.equal``; for the existence forms SEMI and ANTI both -- ANTI is
the same kernel with the flag turned round and is not timed separately).  Reported per form: median, min, max and
inter-quartile range of each and whether (b)'s median lies below (c)'s whole spread -- the rule execute()'s per-form
switch (``_ROW_PREDICATE_FORMS``) follows: a form is on only where that holds at BOTH sizes.  A form's measurement
stops taking repetitions once ``--step-seconds`` have passed (it reports how many it took; fewer than 5 do not count
as faster).  Prints one JSON line per (configuration, form) and a summary line; needs a GPU.

    python tools/row_predicates_timing.py [--configs 1000000x10000000,100000000x10000000] [--reps 10] [--warmup 2]
                                          [--distance 1000] [--step-seconds 120]
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PREDICATES = ("contains", "within", "within_distance")
MIN_REPS = 5


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="1000000x10000000,100000000x10000000",
                    help="left rows x right rows, comma-separated; the larger table is fixed-length 'reads'")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--distance", type=int, default=1000, help="N of DISTANCE(a, b) <= N")
    ap.add_argument("--step-seconds", type=float, default=120.0, help="time limit of one form's repetitions")
    args = ap.parse_args()
    if args.reps < MIN_REPS:
        ap.error(f"--reps must be at least {MIN_REPS}")

    import torch

    from giql_amd import synth
    from giql_amd.engine import DeviceSide, HipEngine

    if not torch.cuda.is_available():
        print("row_predicates_timing: no GPU", file=sys.stderr)
        return 2
    eng = HipEngine(0)

    def side(n, seed, kind):
        c, s, e = synth.make_table(n, seed, kind)
        return DeviceSide.from_numpy(c, s, e, ("0based", "half_open"), device=eng.device)

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

    summary = []
    for cfg in args.configs.split(","):
        n_a, n_b = (int(x) for x in cfg.split("x"))
        # the benchmark's tables (bench.py, cfg4): "peaks" seed 5, "reads" seed 6; the larger side is the reads
        a = side(n_a, 6 if n_a > n_b else 5, "reads" if n_a > n_b else "peaks")
        b = side(n_b, 5 if n_a > n_b else 6, "peaks" if n_a > n_b else "reads")

        def left_ids(predicate):
            if predicate == "contains":
                return eng.contain_join(a, b, 24)[0]
            if predicate == "within":
                return eng.contain_join(b, a, 24)[1]
            return eng.window_join(a, b, 24, args.distance)[0]

        for klass in ("exists", "count"):
            for predicate in PREDICATES:
                md = args.distance if predicate == "within_distance" else None

                if klass == "exists":
                    def new(anti=False):
                        return (eng.semi_anti_pred(a, b, 24, predicate, anti, md),)

                    def composed(anti=False):
                        flags = eng.mark(left_ids(predicate).contiguous(), a.n)
                        return (eng.select([(("a", flags), "=", ("lit", 0 if anti else 1))], n=a.n, n_rows_a=a.n,
                                           want=("a",))[0],)
                else:
                    def new():
                        return (eng.count_pred(a, b, 24, predicate, md),)

                    def composed():
                        return (torch.bincount(left_ids(predicate).long(), minlength=a.n),)

                for _ in range(args.warmup):
                    got, want = new(), composed()
                torch.cuda.synchronize()
                if klass == "exists":                # ANTI is SEMI's kernel with the flag turned round: compared, not timed
                    got, want = got + new(True), want + composed(True)
                equal = all(x.shape == y.shape and bool(torch.equal(x.long(), y.long())) for x, y in zip(got, want))
                n_hit = int(got[0].shape[0]) if klass == "exists" else int((got[0] > 0).sum())
                n_pairs = int(left_ids(predicate).shape[0])
                del got, want
                t = {"new": [], "composed": []}
                t_end = time.perf_counter() + args.step_seconds
                for _ in range(args.reps):           # alternating: both see the same machine
                    for name, fn in (("new", new), ("composed", composed)):
                        ms, out = timed(fn)
                        t[name].append(ms)
                        del out
                    if time.perf_counter() > t_end:
                        break
                s = {k: spread(v) for k, v in t.items()}
                faster = s["new"]["reps"] >= MIN_REPS and s["new"]["median_ms"] < s["composed"]["min_ms"]
                rec = {"rows_a": a.n, "rows_b": b.n, "form": [klass, predicate], "max_distance": md, "n_pairs": n_pairs,
                       "rows_with_a_match": n_hit, "outputs_equal": equal, "new": s["new"], "composed": s["composed"],
                       "new_faster_than_composed": bool(faster)}
                print(json.dumps(rec), flush=True)
                summary.append({"rows_a": a.n, "rows_b": b.n, "form": [klass, predicate], "outputs_equal": equal,
                                "new_faster_than_composed": bool(faster)})
                torch.cuda.empty_cache()
        del a, b
        torch.cuda.empty_cache()
    ok = all(r["outputs_equal"] for r in summary)
    forms = {}
    for r in summary:
        forms.setdefault("/".join(r["form"]), []).append(r["new_faster_than_composed"])
    print(json.dumps({"summary": summary, "all_outputs_equal": ok,
                      "forms_on": {k: all(v) for k, v in forms.items()}}), flush=True)
    eng.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
