"""The one-table and aggregate operators call the library as they did, and launch what they launched, when
``tests/golden/one_table_launches.json`` was recorded -- and answer what the CPU references answer.

CLUSTER and MERGE under a predicate, MERGE with aggregates and STRING_AGG, DISJOIN, the coverage segments and the
aggregates over a join's pairs are built on the host from shared stages: the event sweep of
DISJOIN and coverage, the segmented reduction of MERGE and the pair aggregates, one conversion of the caller's
aggregates, one status-word frame.  Which library entry point a call of the engine takes, and the order and number of
launches per phase and the bytes each phase reports on every path -- one tile of the reduction or several, one sort of
the pairs or two, columns or expression programs, an empty reference, no pairs, no rows, the three-stage sort -- is the
behaviour a rearrangement of those stages has to keep.  ``tools/record_one_table_launches.py`` holds the calls (one
context per group) and recorded the fixture at the commit the file names; it is never regenerated from the code under
test.  Plain CLUSTER / MERGE / DISJOIN are in ``test_sort_driver_launches_gpu.py``, ``group_rows`` in
``test_row_op_launches_gpu.py``."""

import functools
import importlib.util
import json
import os

import numpy as np
import pytest

import _coverage_ref as CV
import _disjoin_ref as DJ
import _merge_agg_ref as MR
import _one_table_ref as OT
import _pair_agg_ref as PR
import _pair_expr_agg_ref as PX
import _string_agg_ref as SR
from oracle import pyoracle as ora

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("record_one_table_launches",
                                               os.path.join(HERE, "..", "tools", "record_one_table_launches.py"))
REC = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(REC)

STEPS = [s for _name, _env, steps in REC.GROUPS for s in steps]


@functools.lru_cache(maxsize=None)
def fixture():
    with open(os.path.join(HERE, "golden", "one_table_launches.json")) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_cases_of_the_list():
    doc = fixture()
    ids = [s["id"] for s in STEPS]
    assert len(ids) == len(set(ids)) and sorted(doc["cases"]) == sorted(ids)
    assert len(doc["recorded_at_commit"]) == 40
    for cid, rec in doc["cases"].items():
        assert set(rec) == {"calls", *REC.STAT_KEYS}, cid
        assert rec["calls"] and all(set(c) == {"fn", "phase_launches", "phase_bytes"} for c in rec["calls"]), cid


# ---------------------------------------------------------------- the CPU references, once per (call, tables)
def _py(name, col):
    """A column of the recorder as Python values, ``None`` = NULL."""
    col = REC.columns(name)[col]
    if isinstance(col, list):
        return col
    values, ok = col
    if values is None:                           # validity alone: any non-NULL value counts
        values = np.ones(ok.shape[0], np.int64)
    return [v if ok is None or ok[i] else None for i, v in enumerate(values.tolist())]


def _lists(name):
    return tuple(x.tolist() for x in REC.table(name))


def _holds(name):
    bit = REC.columns(name)[REC.PRED][0]
    return lambda i, j: bit[i] == bit[j]


@functools.lru_cache(maxsize=None)
def _regions(name, pred):
    return MR.regions(*_lists(name), REC.DISTANCE, _holds(name) if pred else None)


@functools.lru_cache(maxsize=None)
def _layout(name):
    return OT.Layout(*REC.table(name), REC.DISTANCE)


def _nullable(values, valid):
    """The engine's ``(values, valid)`` as a list with ``None`` where the value is NULL."""
    return [v if ok else None for v, ok in zip(values.tolist(), valid.tolist())]


def _check_merge(s, out):
    cid, name, spec = s["id"], s["b"], s["args"].get("aggs", ())
    c, st, en = _lists(name)
    nums = [a for a in spec if a[0] != "STRING_AGG"]
    strs = [a for a in spec if a[0] == "STRING_AGG"]
    pred = "pred" in s["args"]
    holds = _holds(name) if pred else None
    want_num = MR.merge_agg(c, st, en, REC.DISTANCE, {k: _py(name, k) for _f, k in nums}, nums, holds)
    want_str = SR.merge_string_agg(c, st, en, REC.DISTANCE, {a[1]: _py(name, a[1]) for a in strs},
                                   [(a[1], a[2]) for a in strs], holds)
    assert [list(r) for r in zip(*(x.tolist() for x in out[:4]))] == [r[:4] for r in want_num], cid
    assert len(out) == 4 + len(spec), cid
    num_col, str_col = iter(zip(*[r[4:] for r in want_num])), iter(zip(*[r[4:] for r in want_str]))
    L = _layout(name)
    for a, got in zip(spec, out[4:]):
        if a[0] == "STRING_AGG":
            off, data, ok = got
            raw = data.tobytes()
            have = [raw[off[g]:off[g + 1]] if ok[g] else None for g in range(len(want_str))]
            assert have == list(next(str_col)) == L.strings(_py(name, a[1]), a[2]), (cid, a)
        else:
            assert _nullable(*got) == list(next(num_col)), (cid, a)
            values, valid = L.aggregate(a[0], *REC.columns(name)[a[1]])
            assert np.array_equal(got[0], values) and np.array_equal(got[1], valid), (cid, a)


@functools.lru_cache(maxsize=None)
def _pair_reference(a, b, spec):
    """``(pairs, results)`` of ``spec`` over the join of two tables: lists per A row, ``None`` = NULL."""
    row_a, row_b = REC.pairs(a, b)
    n_a = REC.table(a)[0].shape[0]
    ta, tb = REC.table(a), REC.table(b)
    if not any(c == "overlap" for _f, c in spec):
        return PR.pair_aggregate(row_a, row_b, n_a, {c: _py(b, c) for _f, c in spec}, list(spec))
    tree = REC.overlap_tree(ta[1], ta[2], tb[1], tb[2])
    sources = {c: tree if c == "overlap" else ("col", _py(b, c)) for _f, c in spec}
    counts, results, _inputs = PX.pair_expr_aggregate(row_a, row_b, n_a, [(f, sources[c]) for f, c in spec])
    return counts, results


def _check_pairs(s, out):
    cid, spec = s["id"], s["args"]["aggs"]
    counts, results = _pair_reference(s["a"], s["b"], spec)
    assert out[0].tolist() == counts and len(out) == 1 + len(spec), cid
    for (func, col), (values, non_null), want in zip(spec, out[1:], results):
        if func == "COUNT":
            assert values.tolist() == want, (cid, func, col)
        else:                                   # NULL reads 0 with no non-NULL input
            assert [v if k else None for v, k in zip(values.tolist(), non_null.tolist())] == want, (cid, func, col)
            assert not np.any(values[non_null == 0]), (cid, func, col)


def check(s, out):
    op, cid = s["op"], s["id"]
    if op == "cluster":
        want = ora.py_cluster_predicate(*_lists(s["b"]), REC.DISTANCE, _holds(s["b"]))
        assert np.array_equal(out[0], want), cid
    elif op in ("merge", "merge_agg"):
        _check_merge(s, out)
    elif op == "disjoin":
        ref = () if s["a"] is None else REC.table(s["b"])
        target = REC.table(s["b"] if s["a"] is None else s["a"])
        assert np.array_equal(np.stack(out, 1).astype(np.int64), DJ.brute_force_arrays(*target, *ref)), cid
    elif op == "coverage":
        want = CV.sweep_arrays(*REC.table(s["b"]), runs=s["args"]["runs"])
        if s["args"]["with_depth"]:
            assert np.array_equal(np.stack(out, 1).astype(np.int64), want), cid
        else:
            assert out[3] is None and np.array_equal(np.stack(out[:3], 1).astype(np.int64), want[:, :3]), cid
    elif op == "pair_agg":
        _check_pairs(s, out)
    else:
        raise KeyError(op)


def test_the_cases_are_not_trivial():
    """CPU: the tables reach what the case names promise (checked on the references alone)."""
    tile = REC.TILE
    for s in STEPS:
        if s["op"] not in ("merge", "merge_agg"):
            continue
        L = _layout(s["b"])                      # every MERGE case merges some rows and leaves some alone
        assert np.any(L.count > 1) and np.any(L.count == 1), s["id"]
        if s["id"].endswith("one-tile"):
            assert L.n <= tile, s["id"]
        if s["id"].endswith("fold"):             # more than one tile, and a region on both sides of a tile edge
            assert L.n > tile and any(L.region[k - 1] == L.region[k] for k in range(tile, L.n, tile)), s["id"]
    for s in STEPS:
        if "pred" in s["args"]:                  # the predicate splits a region, and not every one
            plain, split = _regions(s["b"], False), _regions(s["b"], True)
            assert len(plain) < len(split) < REC.table(s["b"])[0].shape[0], s["id"]
            ids = ora.py_cluster_predicate(*_lists(s["b"]), REC.DISTANCE, _holds(s["b"]))
            assert not np.array_equal(ids, ora.c_cluster(ora.Side(*REC.table(s["b"])), REC.DISTANCE)), s["id"]
    segments = CV.sweep_arrays(*REC.table("a_abut"))
    runs = CV.sweep_arrays(*REC.table("a_abut"), runs=True)
    assert 0 < runs.shape[0] < segments.shape[0] and len(set(segments[:, 3].tolist())) > 1
    for s in STEPS:
        if s["op"] != "pair_agg":
            continue
        row_a, _row_b = REC.pairs(s["a"], s["b"])
        n, n_a = row_a.shape[0], REC.table(s["a"])[0].shape[0]
        if s["id"].endswith(("no-pairs", "no-a-rows")):
            assert n == 0 and (n_a == 0) == s["id"].endswith("no-a-rows"), s["id"]
        elif s["id"].endswith("one-tile"):
            assert 0 < n <= tile, s["id"]
        else:                                    # more than one tile, and an A row's pairs on both sides of a tile edge
            assert n > tile and any(row_a[k - 1] == row_a[k] for k in range(tile, n, tile)), s["id"]
            assert 0 < len(set(row_a.tolist())) < n_a, s["id"]
    kinds = {c: REC.columns("b_dups")[c][0].dtype.kind for c in ("i32", "f64", "end")}
    assert kinds == {"i32": "i", "f64": "f", "end": "i"}                    # the float SUM alone asks for two sorts
    assert DJ.brute_force_arrays(*REC.table("a"), *REC.table("none")).shape[0] == 0
    assert DJ.brute_force_arrays(*REC.table("b_zero")).shape[0] > REC.table("b_zero")[0].shape[0]    # some rows are cut
    assert DJ.brute_force_arrays(*REC.table("b_mixed"), *REC.table("a_zero")).shape[0] > 0


# ---------------------------------------------------------------- the replay
@pytest.mark.gpu
@pytest.mark.parametrize("group", REC.GROUPS, ids=[g[0] for g in REC.GROUPS])
def test_calls_launches_bytes_and_results(group):
    pytest.importorskip("torch")
    _name, env, steps = group
    recorded = fixture()["cases"]
    for s, out, record in REC.run_group(env, steps):
        print(s["id"], record)
        assert record == recorded[s["id"]], (s["id"], record, recorded[s["id"]])
        check(s, out)
