#!/usr/bin/env python3
"""Time the LEFT OUTER join's pad beside the INNER join and beside the same result composed from older primitives.

Seeded ``synth`` tables over 24 chromosomes, two configurations by default: 1M "peaks" LEFT JOIN 10M "reads", and the
benchmark's own tables with the 100M-row one on the left (100M "reads" LEFT JOIN 10M "peaks").  Three quantities,
ALTERNATING in one process after a warm-up of all three, every repetition device-synchronised:

  (a) ``inner``     ``HipEngine.inner_join``: the pairs alone;
  (b) ``left``      ``HipEngine.left_join``: the pairs written into buffers with room for the left table, then
                    ``giql_hip_left_pad_dev`` appending the unmatched rows in place;
  (c) ``composed``  the same rows from the primitives that were there before: ``inner_join``, ``mark`` (one byte per
                    left row), ``select(flags = 0)`` and ``torch.cat`` of the pairs with the unmatched rows.

The outputs of (b) and (c) are compared as multisets first (sorted 64-bit keys).  Reported: median, min, max and
inter-quartile range of each, (b) - (a) as the cost of padding, and whether (b)'s median lies below (c)'s whole
spread.  Prints one JSON line per configuration and a summary line; needs a GPU.

    python tools/left_join_timing.py [--configs 1000000x10000000,100000000x10000000] [--reps 20] [--warmup 3]
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
    ap.add_argument("--configs", default="1000000x10000000,100000000x10000000",
                    help="left rows x right rows, comma-separated; the larger table is fixed-length 'reads'")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if args.reps < 10:
        ap.error("--reps must be at least 10")

    import torch

    from giql_amd import synth
    from giql_amd.engine import DeviceSide, HipEngine

    if not torch.cuda.is_available():
        print("left_join_timing: no GPU", file=sys.stderr)
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

    def keys(ra, rb):
        return torch.sort((ra.long() << 32) | (rb.long() & 0xFFFFFFFF)).values

    summary = []
    for cfg in args.configs.split(","):
        n_a, n_b = (int(x) for x in cfg.split("x"))
        # the benchmark's tables (bench.py, cfg4): "peaks" seed 5, "reads" seed 6; the larger side is the reads
        a = side(n_a, 6 if n_a > n_b else 5, "reads" if n_a > n_b else "peaks")
        b = side(n_b, 5 if n_a > n_b else 6, "peaks" if n_a > n_b else "reads")

        def inner():
            return eng.inner_join(a, b, 24)

        def left():
            return eng.left_join(a, b, 24)

        def composed():
            ra, rb = eng.inner_join(a, b, 24)
            flags = eng.mark(ra, a.n)
            un = eng.select([(("a", flags), "=", ("lit", 0))], n=a.n, n_rows_a=a.n, want=("a",))[0]
            return torch.cat([ra, un]), torch.cat([rb, torch.full_like(un, -1)])

        for _ in range(args.warmup):
            p, got, want = inner(), left(), composed()
        torch.cuda.synchronize()
        n_pairs, n_total = int(p[0].shape[0]), int(got[0].shape[0])
        equal = n_total == int(want[0].shape[0]) and bool(torch.equal(keys(*got), keys(*want)))
        del p, got, want
        t = {"inner": [], "left": [], "composed": []}
        for _ in range(args.reps):               # alternating: all three see the same machine
            for name, fn in (("inner", inner), ("left", left), ("composed", composed)):
                ms, out = timed(fn)
                t[name].append(ms)
                del out
        s = {k: spread(v) for k, v in t.items()}
        faster = s["left"]["median_ms"] < s["composed"]["min_ms"]
        rec = {"rows_a": a.n, "rows_b": b.n, "n_pairs": n_pairs, "n_padded": n_total - n_pairs, "outputs_equal": equal,
               "inner": s["inner"], "left": s["left"], "composed": s["composed"],
               "pad_cost_ms": round(s["left"]["median_ms"] - s["inner"]["median_ms"], 4),
               "composed_cost_ms": round(s["composed"]["median_ms"] - s["inner"]["median_ms"], 4),
               "left_faster_than_composed": bool(faster)}
        print(json.dumps(rec), flush=True)
        summary.append({"rows_a": a.n, "rows_b": b.n, "outputs_equal": equal, "left_faster_than_composed": bool(faster)})
        del a, b
        torch.cuda.empty_cache()
    ok = all(r["outputs_equal"] for r in summary)
    print(json.dumps({"summary": summary, "all_outputs_equal": ok,
                      "left_faster_everywhere": all(r["left_faster_than_composed"] for r in summary)}), flush=True)
    eng.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
