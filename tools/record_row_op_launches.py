#!/usr/bin/env python
"""Record what the per-row operators launch: tests/golden/row_op_launches.json.

The host paths of SEMI / ANTI / COUNT, NEAREST, group_rows, their CONTAINS / WITHIN / DISTANCE forms and the
within-distance join are lists of launches whose order, phase and count must not move when the host code is
rearranged.  ``giql_hip_stats.phase_launches`` counts them on every call, so a fixed list of small calls, each on a
context whose history is part of the case, pins them: this tool runs ``GROUPS`` and writes the stats of every call.

The fixture is a RECORDED result: run this at the commit whose behaviour is to be kept (``--commit`` names it in the
file), never at the code under test.  ``tests/test_row_op_launches_gpu.py`` imports ``GROUPS``, ``run_group`` and
``STAT_KEYS`` from here, replays the calls, and compares the stats with the fixture and the results with the CPU
references.

    python tools/record_row_op_launches.py --commit $(git rev-parse HEAD) --out tests/golden/row_op_launches.json
"""

import argparse
import functools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_CHROM = 3
SPAN = 300_000
PILE_START, PILE_ROWS = 2_000_000, 40          # a run of more than 32 equal starts (k_fix_start_ties gives up on it)
CLAMP_N = (1 << 33) + 5                        # a widening above the clamp of giql_hip_window_plan_dev
STAT_KEYS = ("n_out", "n_irregular_a", "n_irregular_b", "join_form", "coarse_b", "sort_local", "bucket_bits")


# ---------------------------------------------------------------- the tables: (chrom, start, end), 0-based half-open
def _rows(seed, n, lens):
    r = np.random.default_rng(seed)
    c = r.integers(0, N_CHROM, n)
    s = r.integers(0, SPAN, n)
    ln = np.full(n, lens) if np.isscalar(lens) else r.integers(lens[0], lens[1], n)
    return c.astype(np.int32), s.astype(np.int32), (s + ln).astype(np.int32)


def _with_zero_length(t, seed, k):
    c, s, e = (x.copy() for x in t)
    z = np.random.default_rng(seed).choice(c.size, k, replace=False)
    e[z] = s[z]
    return c, s, e


@functools.lru_cache(maxsize=None)
def table(name):
    if name == "a":
        return _rows(7101, 300, (1, 2000))
    if name == "b_fixed":
        return _rows(7102, 500, 150)
    if name == "b_mixed":
        return _rows(7103, 500, (1, 800))
    if name == "none":
        z = np.zeros(0, np.int32)
        return z, z, z
    if name == "a_zero":
        return _with_zero_length(table("a"), 7104, 20)
    if name == "b_zero":
        return _with_zero_length(table("b_mixed"), 7105, 30)
    if name == "b_dups":                       # rows that share (chrom, start, end): what group_rows groups
        c, s, e = table("b_mixed")
        return np.concatenate([c, c[:60]]), np.concatenate([s, s[:60]]), np.concatenate([e, e[:60]])
    if name == "b_pile":                       # PILE_ROWS equal starts on chromosome 2, ends DESCENDING in input order
        c, s, e = table("b_mixed")
        ps = np.full(PILE_ROWS, PILE_START, np.int32)
        pe = (PILE_START + 4000 - 10 * np.arange(PILE_ROWS)).astype(np.int32)
        return np.concatenate([c, np.full(PILE_ROWS, 2, np.int32)]), np.concatenate([s, ps]), np.concatenate([e, pe])
    if name == "a_pile":                       # with rows whose nearest B rows are the pile's, all at one distance
        c, s, e = table("a")
        qs = (PILE_START - 1000 + 100 * np.arange(5)).astype(np.int32)
        return np.concatenate([c, np.full(5, 2, np.int32)]), np.concatenate([s, qs]), np.concatenate([e, qs + 50])
    raise KeyError(name)


# ---------------------------------------------------------------- the calls
def step(cid, op, a, b, **args):
    return {"id": cid, "op": op, "a": a, "b": b, "args": args}


def _row_groups():
    out = []
    for op in ("semi", "anti", "count"):
        fixed = [step(f"{op}/fixed/first", op, "a", "b_fixed"),             # lengths read back
                 step(f"{op}/fixed/second", op, "a", "b_fixed"),            # speculated
                 step(f"{op}/mixed/after-fixed", op, "a", "b_mixed"),       # the guess misses: the repeat is recorded
                 step(f"{op}/empty-b", op, "a", "none")]
        mixed = [step(f"{op}/mixed/first", op, "a", "b_mixed"),
                 step(f"{op}/mixed/second", op, "a", "b_mixed")]
        if op == "count":
            mixed.append(step("count/zero-length-rows", op, "a_zero", "b_zero"))      # the irregular tail
        out += [(f"{op}-fixed", {}, fixed), (f"{op}-mixed", {}, mixed)]
    local = [step("local/semi/fixed", "semi", "a", "b_fixed"), step("local/anti/mixed", "anti", "a", "b_mixed"),
             step("local/count/mixed", "count", "a", "b_mixed"), step("local/count/fixed", "count", "a", "b_fixed")]
    out.append(("row-three-stage-sort", {"GIQL_HIP_LOCAL_MIN_ROWS": "1"}, local))
    return out


def _nearest_groups():
    k1 = [step("nearest/first", "nearest", "a", "b_mixed"),                 # the layout probe
          step("nearest/second", "nearest", "a", "b_mixed"),                # keys from the raw columns
          step("nearest32", "nearest32", "a", "b_mixed"),
          step("nearest/pile/first", "nearest", "a_pile", "b_pile"),        # flags the two-sort plan and repeats
          step("nearest/pile/second", "nearest", "a_pile", "b_pile")]       # the two-sort plan from the start
    kn = [step("nearest-k3/one-sort", "nearest_k", "a", "b_mixed", k=3),
          step("nearest-k16/one-sort", "nearest_k", "a", "b_mixed", k=16),
          step("nearest-k3/pile/first", "nearest_k", "a_pile", "b_pile", k=3),
          step("nearest-k3/two-sorts", "nearest_k", "a_pile", "b_pile", k=3),
          step("nearest-k16/two-sorts", "nearest_k", "a", "b_mixed", k=16)]
    gr = [step("group-rows/one-sort", "group_rows", None, "b_dups"),
          step("group-rows/pile/first", "group_rows", None, "b_pile"),
          step("group-rows/two-sorts", "group_rows", None, "b_dups")]
    return [("nearest", {}, k1), ("nearest-k", {}, kn), ("group-rows", {}, gr)]


def _pred_groups():
    semi, count = [], []
    for pred in ("contains", "within"):
        for anti in (False, True):
            semi.append(step(f"{'anti' if anti else 'semi'}-pred/{pred}", "semi_pred", "a", "b_mixed", predicate=pred, anti=anti))
        semi.append(step(f"anti-pred/{pred}/empty-b", "semi_pred", "a", "none", predicate=pred, anti=True))
        count.append(step(f"count-pred/{pred}", "count_pred", "a_zero", "b_zero", predicate=pred))
        count.append(step(f"count-pred/{pred}/empty-b", "count_pred", "a", "none", predicate=pred))
    for n in (0, 1000, -1):
        for anti in (False, True):
            semi.append(step(f"{'anti' if anti else 'semi'}-pred/within-distance/{n}", "semi_pred", "a_zero", "b_zero",
                             predicate="within_distance", anti=anti, max_distance=n))
        count.append(step(f"count-pred/within-distance/{n}", "count_pred", "a_zero", "b_zero",
                          predicate="within_distance", max_distance=n))
    semi.append(step("semi-pred/within-distance/empty-b", "semi_pred", "a", "none", predicate="within_distance",
                     anti=False, max_distance=5))
    count.append(step("count-pred/within-distance/empty-b", "count_pred", "a", "none", predicate="within_distance",
                      max_distance=5))
    window = [step("window-join/1000", "window_join", "a_zero", "b_zero", max_distance=1000),
              step("window-join/clamp", "window_join", "a_zero", "b_zero", max_distance=CLAMP_N)]
    return [("semi-anti-pred", {}, semi), ("count-pred", {}, count), ("window-join", {}, window)]


GROUPS = _row_groups() + _nearest_groups() + _pred_groups()      # (name, environment of the context, its calls in order)


def make_engine(env):
    """A context created under ``env`` (the switches are read once, at giql_hip_create)."""
    from giql_amd.engine import HipEngine

    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return HipEngine(0)
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def device_side(name):
    from giql_amd.engine import DeviceSide

    return DeviceSide.from_numpy(*table(name))


def run_step(eng, s):
    """One call; its results as numpy arrays (a tuple) and the statistics the fixture keeps."""
    op, args = s["op"], s["args"]
    b = device_side(s["b"])
    a = device_side(s["a"]) if s["a"] else None
    if op in ("semi", "anti"):
        out = (eng.semi_anti(a, b, N_CHROM, op == "anti"),)
    elif op == "count":
        out = (eng.count_overlaps(a, b, N_CHROM),)
    elif op == "nearest":
        out = eng.nearest(a, b, N_CHROM)
    elif op == "nearest32":
        out = (eng.nearest32(a, b, N_CHROM),)
    elif op == "nearest_k":
        out = eng.nearest_k(a, b, N_CHROM, args["k"])
    elif op == "group_rows":
        out = eng.group_rows(b, N_CHROM)
    elif op == "semi_pred":
        out = (eng.semi_anti_pred(a, b, N_CHROM, args["predicate"], args["anti"], args.get("max_distance")),)
    elif op == "count_pred":
        out = (eng.count_pred(a, b, N_CHROM, args["predicate"], args.get("max_distance")),)
    elif op == "window_join":
        out = eng.window_join(a, b, N_CHROM, args["max_distance"])
    else:
        raise KeyError(op)
    st = eng.stats()
    record = {"phase_launches": {k: v for k, v in st["phase_launches"].items() if v}}
    record.update({k: st[k] for k in STAT_KEYS})
    return tuple(t.cpu().numpy() for t in out), record


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
           "note": "recorded by tools/record_row_op_launches.py at the commit above; never regenerated from the code under test",
           "cases": cases}
    with open(ns.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(cases)} calls recorded at {ns.commit} -> {ns.out}")


if __name__ == "__main__":
    main()
