#!/usr/bin/env python
"""Record what the one-table and aggregate operators launch: tests/golden/one_table_launches.json.

``record_row_op_launches.py`` pins the per-row operators and ``record_sort_driver_launches.py`` plain CLUSTER / MERGE /
DISJOIN.  This one pins the rest of the family, whose host paths share their stages: CLUSTER and
MERGE under a predicate, MERGE with aggregates (one tile of the segmented reduction, and more than one), MERGE with
STRING_AGG, DISJOIN in both modes and against an empty reference, the coverage segments, and the aggregates over a
join's pairs (one sort or two, columns or expressions, one tile or more, no pairs, no rows).

A call of the engine may be several calls of the library (the STRING_AGG plan and its fills, DISJOIN's plan and fill),
and which entry point a call takes is part of what is pinned.  So a record is the list of the library calls of one
step, each with its non-zero ``phase_launches`` and ``phase_bytes``, plus a few statistics of the last one.

The fixture is a RECORDED result: run this at the commit whose behaviour is to be kept (``--commit`` names it in the
file), never at the code under test.  ``tests/test_one_table_launches_gpu.py`` imports ``GROUPS`` and ``run_group``
from here, replays the calls, and compares the records with the fixture and the results with the CPU references.  The
tables, ``make_engine`` and ``step`` are ``record_row_op_launches.py``'s.

    python tools/record_one_table_launches.py --commit $(git rev-parse HEAD) --out tests/golden/one_table_launches.json
"""

import argparse
import functools
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

_spec = importlib.util.spec_from_file_location("record_row_op_launches", os.path.join(HERE, "record_row_op_launches.py"))
ROWS = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ROWS)

N_CHROM = ROWS.N_CHROM
step = ROWS.step
make_engine = ROWS.make_engine
STAT_KEYS = ("n_out", "sort_local", "bucket_bits")
DISTANCE = 200                                  # at this distance a region of b_mixed crosses the reduction's tile edge
TILE = 256                                      # MAGG_TILE: the rows (or pairs) one block of the reduction takes
SMALL_ROWS = 200


# ---------------------------------------------------------------- the tables: the row operators', and two derived ones
@functools.lru_cache(maxsize=None)
def table(name):
    if name == "b_small":                       # one tile of the segmented reduction
        return tuple(x[:SMALL_ROWS] for x in ROWS.table("b_mixed"))
    if name == "a_abut":                        # rows that start where another ends: segments of equal depth abut
        c, s, e = ROWS.table("a")
        return np.concatenate([c, c[:60]]), np.concatenate([s, e[:60]]), np.concatenate([e, e[:60] + 100])
    return ROWS.table(name)


@functools.lru_cache(maxsize=None)
def columns(name):
    """The value columns of a table, per row: name -> ``(values, valid or None)``; a string column is a list of
    ``bytes | None``.  The floats are multiples of 1/4 below 2^10: a sum of them is exact in any order."""
    n = table(name)[0].shape[0]
    r = np.random.default_rng(7200 + n)
    i32 = r.integers(-1000, 1000, n).astype(np.int32)
    ok = r.random(n) >= 0.1
    f64 = r.integers(-4096, 4096, n).astype(np.float64) / 4
    kind = r.random(n)
    names = [None if k < 0.1 else b"" if k < 0.15 else b"n%d" % i for i, k in enumerate(kind.tolist())]
    tags = [b"x%d" % (i % 7) for i in range(n)]
    return {"i32": (i32, ok), "f64": (f64, None), "end": (table(name)[2], None), "valid": (None, ok),
            "bit": (r.integers(0, 2, n).astype(np.int32), None), "names": names, "tags": tags}


def overlap_tree(a_start, a_end, b_start, b_end):
    """``overlap_bp`` of a pair as an expression tree over the four columns (numpy arrays or device tensors)."""
    return ("-", ("least", ("a", a_end), ("b", b_end)), ("greatest", ("a", a_start), ("b", b_start)))


@functools.lru_cache(maxsize=None)
def pairs(a, b):
    """The INNER join's pairs of two tables, ordered: int32 ``(row_a, row_b)``."""
    from oracle import pyoracle as ora

    if 0 in (table(a)[0].shape[0], table(b)[0].shape[0]):
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    p = ora.sort_pairs(*ora.c_inner(ora.Side(*table(a)), ora.Side(*table(b)), "sweep"))
    return p[:, 0].astype(np.int32), p[:, 1].astype(np.int32)


# ---------------------------------------------------------------- the calls
NUMERIC = (("SUM", "i32"), ("AVG", "i32"), ("MAX", "end"), ("SUM", "f64"), ("COUNT", "i32"))     # AVG shares the SUM
PRED = "bit"                                    # predicate := bit = PREV(bit)

PAIR_INT = (("SUM", "i32"), ("MAX", "end"), ("COUNT", "valid"), ("AVG", "i32"))
PAIR_FLOAT = (("SUM", "f64"),)
PAIR_EXPR = (("SUM", "overlap"), ("MAX", "overlap"))
PAIR_BOTH = (("SUM", "i32"), ("SUM", "overlap"), ("MIN", "f64"))


def _merge_steps(p, small, large):
    return [step(f"{p}merge-agg/one-tile", "merge_agg", None, small, aggs=NUMERIC),
            step(f"{p}merge-agg/fold", "merge_agg", None, large, aggs=NUMERIC)]


def _pair_steps(p, b):
    return [step(f"{p}pair-agg/float-sum", "pair_agg", "a", b, aggs=PAIR_FLOAT)]        # two sorts


GROUPS = [        # (name, environment of the context, its calls in order)
    ("cluster-merge", {}, [step("cluster/pred", "cluster", None, "b_mixed", pred=PRED),
                           step("merge/pred", "merge", None, "b_mixed", pred=PRED)]
     + _merge_steps("", "b_small", "b_mixed")
     + [step("merge-str/one", "merge_agg", None, "b_mixed", aggs=(("MIN", "i32"), ("STRING_AGG", "names", b","))),
        step("merge-str/two-and-sum", "merge_agg", None, "b_mixed",
             aggs=(("STRING_AGG", "names", b","), ("SUM", "i32"), ("STRING_AGG", "tags", b"; "))),
        step("merge-str/only", "merge_agg", None, "b_mixed", aggs=(("STRING_AGG", "tags", b""),))]),   # no MaggArgs
    ("disjoin", {}, [step("disjoin/self", "disjoin", None, "b_zero"),
                     step("disjoin/reference", "disjoin", "b_mixed", "a_zero"),              # a = target, b = reference
                     step("disjoin/empty-reference", "disjoin", "a", "none")]),              # no event at all
    ("coverage", {}, [step("coverage/segments", "coverage", None, "a_abut", runs=False, with_depth=True),
                      step("coverage/runs", "coverage", None, "a_abut", runs=True, with_depth=True),
                      step("coverage/no-depth", "coverage", None, "a_abut", runs=False, with_depth=False)]),
    ("pair-agg", {}, [step("pair-agg/int", "pair_agg", "a", "b_dups", aggs=PAIR_INT),        # one sort; more than a tile
                      step("pair-agg/int/one-tile", "pair_agg", "a", "b_mixed", aggs=PAIR_INT)]
     + _pair_steps("", "b_dups")
     + [step("pair-agg/expr", "pair_agg", "a", "b_dups", aggs=PAIR_EXPR),
        step("pair-agg/expr/one-tile", "pair_agg", "a", "b_mixed", aggs=PAIR_EXPR),
        step("pair-agg/columns-and-expr", "pair_agg", "a", "b_dups", aggs=PAIR_BOTH),
        step("pair-agg/no-aggregates", "pair_agg", "a", "b_dups", aggs=()),
        step("pair-agg/no-pairs", "pair_agg", "a", "none", aggs=PAIR_INT),
        step("pair-agg/no-a-rows", "pair_agg", "none", "b_mixed", aggs=PAIR_INT)]),
    ("one-table-three-stage-sort", {"GIQL_HIP_LOCAL_MIN_ROWS": "1"},
     _merge_steps("local/", "b_small", "b_mixed")
     + [step("local/coverage/segments", "coverage", None, "a_abut", runs=False, with_depth=True)]
     + _pair_steps("local/", "b_dups")),
]


class _Spy:
    """The library as the engine sees it, noting after every device call what that call launched."""

    def __init__(self, eng):
        self._eng, self._lib, self.calls = eng, eng._L, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.endswith("_dev"):
            return fn

        def call(*args):
            rc = fn(*args)
            st = self._eng.stats()
            self.calls.append({"fn": name,
                               "phase_launches": {k: v for k, v in st["phase_launches"].items() if v},
                               "phase_bytes": {k: v for k, v in st["phase_bytes"].items() if v}})
            return rc

        return call


@functools.lru_cache(maxsize=None)
def device_side(name):
    from giql_amd.engine import DeviceSide

    return DeviceSide.from_numpy(*table(name))


@functools.lru_cache(maxsize=None)
def device_columns(name):
    """``columns(name)`` on the device; a string column as ``(offsets, data, valid)`` in the utf8 layout."""
    import torch

    def dev(x):
        return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")

    out = {}
    for k, col in columns(name).items():
        if isinstance(col, list):
            off = np.concatenate([[0], np.cumsum([len(v or b"") for v in col])]).astype(np.int32)
            data = np.frombuffer(b"".join(v or b"" for v in col), np.uint8).copy()
            out[k] = (dev(off), dev(data), dev(np.array([v is not None for v in col], np.uint8)))
        else:
            out[k] = (dev(col[0]), None if col[1] is None else dev(col[1].astype(np.uint8)))
    return out


def _merge_aggs(spec, cols):
    return [("STRING_AGG",) + cols[a[1]] + (a[2],) if a[0] == "STRING_AGG" else (a[0],) + cols[a[1]] for a in spec]


def _pair_aggs(spec, a, b):
    """The engine's entries for ``spec`` over the tables named ``a`` and ``b``."""
    cols, sa, sb = device_columns(b), device_side(a), device_side(b)
    tree = overlap_tree(sa.start, sa.end, sb.start, sb.end)
    return [(f, ("expr", tree)) if c == "overlap" else (f,) + cols[c] for f, c in spec]


def run_step(eng, s):
    """One call; its results as numpy arrays (a tuple, nested where the engine's is) and the record the fixture keeps."""
    import torch

    op, args = s["op"], s["args"]
    b = device_side(s["b"])
    spy = _Spy(eng)
    eng._L = spy
    try:
        if op in ("cluster", "merge"):
            bit = device_columns(s["b"])[args["pred"]][0]
            preds = [(("a", bit), "=", ("b", bit))]
            out = (eng.cluster(b, N_CHROM, DISTANCE, preds),) if op == "cluster" else eng.merge(b, N_CHROM, DISTANCE, preds)
        elif op == "merge_agg":
            out = eng.merge_agg(b, N_CHROM, DISTANCE, _merge_aggs(args["aggs"], device_columns(s["b"])))
        elif op == "disjoin":
            out = eng.disjoin(b, None, N_CHROM) if s["a"] is None else eng.disjoin(device_side(s["a"]), b, N_CHROM)
        elif op == "coverage":
            out = eng.coverage(b, N_CHROM, runs=args["runs"], with_depth=args["with_depth"])
        elif op == "pair_agg":
            a = device_side(s["a"])
            ra, rb = (torch.from_numpy(x).to("cuda:0") for x in pairs(s["a"], s["b"]))
            counts, res = eng.pair_aggregate(ra, rb, a.n, b.n, _pair_aggs(args["aggs"], s["a"], s["b"]))
            out = (counts,) + tuple(res)
        else:
            raise KeyError(op)
    finally:
        eng._L = spy._lib
    st = eng.stats()
    record = {"calls": spy.calls}
    record.update({k: st[k] for k in STAT_KEYS})

    def host(x):
        return None if x is None else tuple(host(y) for y in x) if isinstance(x, (tuple, list)) else x.cpu().numpy()

    return host(out), record


def run_group(env, steps):
    """The calls of one group on one fresh context: ``[(step, results, record), ...]``."""
    eng = make_engine(env)
    try:
        return [(s,) + run_step(eng, s) for s in steps]
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--commit", required=True, help="hash of the commit this runs at (written into the file)")
    ap.add_argument("--out", required=True)
    ns = ap.parse_args()
    cases = {}
    for _name, env, steps in GROUPS:
        for s, _out, record in run_group(env, steps):
            assert s["id"] not in cases, s["id"]
            cases[s["id"]] = record
    doc = {"recorded_at_commit": ns.commit,
           "note": "recorded by tools/record_one_table_launches.py at the commit above; never regenerated from the code under test",
           "cases": cases}
    with open(ns.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(cases)} calls recorded at {ns.commit} -> {ns.out}")


if __name__ == "__main__":
    main()
