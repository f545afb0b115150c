#!/usr/bin/env python
"""Record what the callers of the sort driver launch: tests/golden/sort_driver_launches.json.

``record_row_op_launches.py`` pins the per-row operators.  This one pins every other path through the host driver of
the sort (``run_sort_onesweep`` / ``run_linearize`` in giql_hip.hip): the INNER plan and the one-call join in their
general, fixed-length, exchanged, presorted and irregular forms, with two, three and four global passes, the fused
count and the join in the bucket stage, the classic sort and another block shape, the index build and the operators
that read an index, CLUSTER / MERGE / DISJOIN, and the CONTAINS join.  Besides ``phase_launches`` it keeps
``phase_bytes``: the algorithmic bytes a sort reports are decided by the same host code as its launches.

The fixture is a RECORDED result: run this at the commit whose behaviour is to be kept (``--commit`` names it in the
file), never at the code under test.  ``tests/test_sort_driver_launches_gpu.py`` imports ``GROUPS`` and ``run_group``
from here, replays the calls, and compares the stats with the fixture and the results with the CPU references.  The
tables, ``make_engine`` and ``step`` are ``record_row_op_launches.py``'s.

    python tools/record_sort_driver_launches.py --commit $(git rev-parse HEAD) --out tests/golden/sort_driver_launches.json
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
STAT_KEYS = ("join_form", "span_hist", "sort_local", "bucket_bits", "n_out", "n_irregular_a", "n_irregular_b")
CLUSTER_DISTANCE = 50


# ---------------------------------------------------------------- the tables: the row operators', and two sorted copies
@functools.lru_cache(maxsize=None)
def table(name):
    if name.endswith("_sorted"):                # in (chrom, start) order: the side's sort is skipped once that is known
        c, s, e = ROWS.table(name[: -len("_sorted")])
        order = np.lexsort((s, c))
        return c[order], s[order], e[order]
    return ROWS.table(name)


@functools.lru_cache(maxsize=None)
def device_side(name):
    from giql_amd.engine import DeviceSide

    return DeviceSide.from_numpy(*table(name))


# ---------------------------------------------------------------- the calls
def _inner_steps(p):
    return [step(f"{p}/mixed/first", "plan_fill", "a", "b_mixed"),           # general form; lengths read back
            step(f"{p}/mixed/second", "join_into", "a", "b_mixed"),          # speculated
            step(f"{p}/fixed/plan-fill", "plan_fill", "a", "b_fixed"),       # the guess of the form misses: repeated
            step(f"{p}/fixed/join-1", "join_into", "a", "b_fixed"),          # speculated fixed-length form
            step(f"{p}/fixed/join-2", "join_into", "a", "b_fixed"),          # settled: early fill / bucket-stage join
            step(f"{p}/fixed/exchanged", "join_into", "b_fixed", "a"),
            step(f"{p}/sorted/first", "join_into", "a_sorted", "b_fixed_sorted"),
            step(f"{p}/sorted/second", "join_into", "a_sorted", "b_fixed_sorted"),   # skips the sorts
            step(f"{p}/zero-length-rows", "join_into", "a_zero", "b_zero")]  # the irregular tail


def _switch_steps(p):
    return [step(f"{p}/fixed/first", "plan_fill", "a", "b_fixed"),
            step(f"{p}/fixed/second", "join_into", "a", "b_fixed"),
            step(f"{p}/general", "join_into", "a", "b_mixed")]


def _index_steps(p):
    out = []
    for t in ("b_fixed", "b_mixed"):
        out += [step(f"{p}/{t}/create", "index_create", None, t),            # the stats of the build itself
                step(f"{p}/{t}/inner-join", "inner_join_indexed", "a", t),
                step(f"{p}/{t}/count", "count_indexed", "a", t),             # prepares the rows: the end sort
                step(f"{p}/{t}/nearest", "nearest_indexed", "a", t)]
    return out


THREE_STAGE = {"GIQL_HIP_LOCAL_MIN_ROWS": "1"}
NARROW = {"GIQL_HIP_LOCAL_MIN_ROWS": "1", "GIQL_HIP_LOCAL_BITS": "13"}

GROUPS = [        # (name, environment of the context, its calls in order)
    ("inner", {}, _inner_steps("inner")),
    ("inner-three-stage", THREE_STAGE, _inner_steps("inner3")),
    ("inner-narrow", NARROW, [step("narrow/mixed", "plan_fill", "a", "b_mixed"),
                              step("narrow/mixed/second", "join_into", "a", "b_mixed"),
                              step("narrow/fixed", "plan_fill", "a", "b_fixed"),
                              step("narrow/fixed/second", "join_into", "a", "b_fixed"),
                              step("narrow/fixed/third", "join_into", "a", "b_fixed")]),
    ("inner-no-span-hist", {"GIQL_HIP_NO_SPAN_HIST": "1"}, _switch_steps("no-span-hist")),
    ("inner-no-fuse-count", dict(THREE_STAGE, GIQL_HIP_NO_FUSE_COUNT="1"), _switch_steps("no-fuse-count")),
    ("inner-classic-sort", {"GIQL_HIP_SORT": "classic"}, _switch_steps("classic")),
    ("inner-os-variant-3", {"GIQL_HIP_OS_VARIANT": "3"}, _switch_steps("os-variant-3")),
    ("index", {}, _index_steps("index")),
    ("index-narrow", {"GIQL_HIP_LOCAL_BITS": "13"}, _index_steps("index13")),
    ("one-table", {}, [step("cluster", "cluster", None, "b_mixed"),
                       step("merge", "merge", None, "b_mixed"),
                       step("disjoin/self", "disjoin", None, "a"),
                       step("disjoin/reference", "disjoin", "a", "b_mixed")]),      # a = target, b = reference
    ("contains", {}, [step("contains/general", "contain_join", "a", "b_mixed"),
                      step("contains/uniform-inner", "contain_join", "a", "b_fixed")]),
]


def run_step(eng, s, state):
    """One call; its results as numpy arrays (a tuple) and the statistics the fixture keeps.  ``state`` lives as long
    as the group's context: the index a later call of the group reads."""
    import torch

    op = s["op"]
    b = device_side(s["b"])
    a = device_side(s["a"]) if s["a"] else None
    i32 = dict(dtype=torch.int32, device=b.start.device)
    if op == "plan_fill":
        n = eng.inner_plan(a, b, N_CHROM)
        out = (torch.empty(n, **i32), torch.empty(n, **i32))
        eng.inner_fill(*out)
    elif op == "join_into":                      # room for every pair there can be: never GIQL_ERR_CAPACITY
        ra, rb = torch.empty(a.n * b.n, **i32), torch.empty(a.n * b.n, **i32)
        n = eng.inner_join_into(a, b, N_CHROM, ra, rb)
        out = (ra[:n], rb[:n])
    elif op == "index_create":
        if state.get("index") is not None:
            state["index"].close()
        state["index"] = eng.index_create(b, N_CHROM)
        out = ()
    elif op == "inner_join_indexed":
        out = eng.inner_join_indexed(a, state["index"], cap=a.n * b.n)
    elif op == "count_indexed":
        out = (eng.count_overlaps_indexed(a, state["index"]),)
    elif op == "nearest_indexed":
        out = eng.nearest_indexed(a, state["index"])
    elif op == "cluster":
        out = (eng.cluster(b, N_CHROM, CLUSTER_DISTANCE),)
    elif op == "merge":
        out = eng.merge(b, N_CHROM, CLUSTER_DISTANCE)
    elif op == "disjoin":
        out = eng.disjoin(b, None, N_CHROM) if a is None else eng.disjoin(a, b, N_CHROM)
    elif op == "contain_join":
        out = eng.contain_join(a, b, N_CHROM)
    else:
        raise KeyError(op)
    st = eng.stats()
    record = {"phase_launches": {k: v for k, v in st["phase_launches"].items() if v},
              "phase_bytes": {k: v for k, v in st["phase_bytes"].items() if v}}
    record.update({k: st[k] for k in STAT_KEYS})
    return tuple(t.cpu().numpy() for t in out), record


def run_group(env, steps):
    """The calls of one group on one fresh context: ``[(step, results, record), ...]``."""
    eng = make_engine(env)
    state = {}
    try:
        return [(s,) + run_step(eng, s, state) for s in steps]
    finally:
        if state.get("index") is not None:
            state["index"].close()
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
           "note": "recorded by tools/record_sort_driver_launches.py at the commit above; never regenerated from the code under test",
           "cases": cases}
    with open(ns.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(cases)} calls recorded at {ns.commit} -> {ns.out}")


if __name__ == "__main__":
    main()
