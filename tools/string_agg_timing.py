"""MERGE, merge_agg and STRING_AGG beside MERGE on the `reads` table of the headline workload (synth, 100M rows, seed 6,
24 chromosomes) plus a seeded string column of 8-12 bytes per row and a float64 score: 2 warm-ups, then the median of 5
calls, each ending in a device synchronise ("STRING_AGG beside MERGE").

usage: string_agg_timing.py TREE LINES [N]
TREE   directory holding the giql_amd package to import (this checkout, or an export of another commit with its
       library built: the lines a and b exist in both)
LINES  letters: a eng.merge; b eng.merge_agg with one COUNT; c one STRING_AGG(name, ',') and the context's phase events
       of its two calls; d c plus SUM(score); e the host route (eng.cluster, ids to the host, pyarrow hash_list, then
       binary_join)."""
import json
import statistics
import sys
import time

tree, lines = sys.argv[1], sys.argv[2]
N = int(sys.argv[3]) if len(sys.argv) > 3 else 100_000_000
sys.path.insert(0, tree)

import numpy as np
import torch

import giql_amd
from giql_amd import synth
from giql_amd.engine import DeviceSide, HipEngine

assert giql_amd.__file__.startswith(tree), giql_amd.__file__
t0 = time.time()
c, s, e = synth.make_table(N, 6, "reads")
n_chrom = 24
rng = np.random.default_rng(6)
strings = any(k in lines for k in "cde")
lens = rng.integers(8, 13, N if strings else 1).astype(np.int64)
off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
data = rng.integers(97, 123, int(off[-1]), dtype=np.uint8)
score = rng.normal(0, 100, N if strings else 1)
print(f"[setup] {N} rows, {int(off[-1])} name bytes, {time.time() - t0:.1f} s", flush=True)
eng = HipEngine(0)
side = DeviceSide.from_numpy(c, s, e)
dev = "cuda:0"
off_d, data_d, score_d = torch.from_numpy(off).to(dev), torch.from_numpy(data).to(dev), torch.from_numpy(score).to(dev)


def timed(fn, warm=2, reps=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
        del out
    return statistics.median(ts), ts


def report(name, fn, **kw):
    med, ts = timed(fn, **kw)
    print(json.dumps({"line": name, "tree": tree, "median_ms": round(med, 3), "all_ms": [round(t, 3) for t in ts]}), flush=True)


if "a" in lines:
    report("a eng.merge", lambda: eng.merge(side, n_chrom, 0))
if "b" in lines:
    report("b eng.merge_agg COUNT", lambda: eng.merge_agg(side, n_chrom, 0, [("COUNT", side.start, None)]))
if "c" in lines:
    one = [("STRING_AGG", off_d, data_d, None, ",")]
    report("c STRING_AGG(name, ',')", lambda: eng.merge_agg(side, n_chrom, 0, one))
    out = eng.merge_agg(side, n_chrom, 0, one)
    print(json.dumps({"regions": int(out[0].numel()), "out_bytes": int(out[4][1].numel())}), flush=True)
    del out
    # the context's phase events of the two calls behind (c)
    eng.set_profiling(True)
    real = eng._L.giql_hip_concat_utf8_fill_dev
    seen = {}

    def spy(*args):
        seen["plan"] = eng.stats()
        rc = real(*args)
        seen["fill"] = eng.stats()
        return rc

    eng._L.giql_hip_concat_utf8_fill_dev = spy
    for _ in range(3):
        eng.merge_agg(side, n_chrom, 0, one)
        torch.cuda.synchronize()
    eng._L.giql_hip_concat_utf8_fill_dev = real
    eng.set_profiling(False)
    for k in ("plan", "fill"):
        st = seen[k]
        print(json.dumps({"phases of": k, "total_ms": round(st["total_ms"], 3),
                          "phase_ms": {p: round(v, 3) for p, v in st["phase_ms"].items() if v},
                          "launches": {p: v for p, v in st["phase_launches"].items() if v}}), flush=True)
if "d" in lines:
    report("d STRING_AGG + SUM(score)", lambda: eng.merge_agg(side, n_chrom, 0, [("STRING_AGG", off_d, data_d, None, ","),
                                                                                  ("SUM", score_d, None)]))
if "e" in lines:
    import pyarrow as pa
    import pyarrow.compute as pc

    names = pa.Array.from_buffers(pa.string(), N, [None, pa.py_buffer(off), pa.py_buffer(data)])
    chrom = pa.array(c)

    def host_route():
        ids = eng.cluster(side, n_chrom, 0).cpu().numpy()
        t = pa.table({"chrom": chrom, "id": pa.array(ids), "name": names})
        g = t.group_by(["chrom", "id"], use_threads=True).aggregate([("name", "list")])
        return pc.binary_join(g.column("name_list"), ",")

    report("e host route", host_route)
