"""Grouped aggregates over a join in the map shape (``join_aggregates=True``; bedtools ``map``): the two routing
decisions, what the flag changes and what it leaves alone, the string form, the overflow guard, the numpy reference
against the sqlite-minted rows, and the C ABI's declaration.  The GPU halves are tests/test_pair_agg_gpu.py (the
kernels) and tests/test_join_aggregates_gpu.py (``execute``)."""
import inspect
import json
import os
import re
from dataclasses import replace

import numpy as np
import pyarrow as pa
import pytest

import _join_agg_queries as Q
import _pair_agg_ref as R
from giql_amd import _lib, execute as X
from giql_amd.plan import JoinPlan, PlanSide
from giql_amd.shape import ColRef, JoinShape, SelItem, TableRef, is_map_shape, map_aggregate_ok
from giql_amd.transpile import build_plan, transpile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
GOLDEN = json.load(open(os.path.join(HERE, "golden", "join_aggregates.json")))
RECORDED = json.load(open(os.path.join(HERE, "golden", "join_aggregates_plans.json")))


# ---------------------------------------------------------------- the routing decision on the parsed shape
A, B = PlanSide("a", "a"), PlanSide("b", "b")


def col(table, column):
    return ColRef(table, False, column)


def agg(func, table="b", column="score", alias="x", distinct=False):
    return SelItem(None if table is None else col(table, column), alias, func, distinct)


SPATIAL = ("intersects", col("a", "interval"), col("b", "interval"))
RESIDUAL = ("cmp", ("col", col("a", "strand")), "=", ("col", col("b", "strand")))


def shape(**kw):
    base = dict(items=[SelItem(col("a", "name")), agg("SUM")], from_ref=TableRef("a", "a"), join_ref=TableRef("b", "b"),
                kind="INNER", on_seen=True, on_terms=[SPATIAL], group_by=[col("a", "name")], join_aggregates=True)
    base.update(kw)
    return JoinShape(**base)


def test_the_shape_routes_over_every_clause():
    assert is_map_shape(shape(), A, B)
    assert not is_map_shape(shape(join_aggregates=False), A, B)
    # the join
    assert is_map_shape(shape(kind="LEFT"), A, B)
    assert is_map_shape(shape(kind="LEFT", on_terms=[SPATIAL, RESIDUAL]), A, B)
    assert is_map_shape(shape(on_terms=[], where_terms=[SPATIAL, RESIDUAL]), A, B)           # INNER: WHERE is a filter
    assert not is_map_shape(shape(kind="LEFT", where_terms=[RESIDUAL]), A, B)               # LEFT: no WHERE
    assert not is_map_shape(shape(kind="LEFT", on_terms=[RESIDUAL], where_terms=[SPATIAL]), A, B)
    for kind in ("SEMI", "ANTI", "COUNT"):
        assert not is_map_shape(shape(kind=kind), A, B)
    for pred in ("contains", "within"):
        assert is_map_shape(shape(on_terms=[(pred,) + SPATIAL[1:]]), A, B)
    assert is_map_shape(shape(on_terms=[("within_distance",) + SPATIAL[1:] + (100,)]), A, B)
    # GROUP BY
    assert not is_map_shape(shape(group_by=[]), A, B)
    assert not is_map_shape(shape(group_by=[col("b", "name")]), A, B)
    assert not is_map_shape(shape(group_by=[col(None, "name")]), A, B)
    assert not is_map_shape(shape(group_by=[col("a", "name"), col("b", "name")]), A, B)
    assert is_map_shape(shape(group_by=[col("a", "name"), col("a", "chrom")]), A, B)
    # plain columns
    assert not is_map_shape(shape(items=[SelItem(col("a", "score")), agg("SUM")]), A, B)     # not a key
    assert not is_map_shape(shape(items=[SelItem(col("b", "name")), agg("SUM")]), A, B)
    assert not is_map_shape(shape(items=[SelItem(ColRef("a", False, "*", star=True)), agg("SUM")]), A, B)
    assert is_map_shape(shape(items=[agg("SUM")]), A, B)                                    # a hidden key
    # aggregates
    for func in ("COUNT", "SUM", "AVG", "MIN", "MAX"):
        assert is_map_shape(shape(items=[agg(func)]), A, B)
    assert is_map_shape(shape(items=[agg("COUNT", None)]), A, B)                            # COUNT(*)
    assert not is_map_shape(shape(items=[agg("SUM", None)]), A, B)
    assert not is_map_shape(shape(items=[agg("SUM", "a")]), A, B)
    assert not is_map_shape(shape(items=[agg("COUNT", "a")]), A, B)
    assert not is_map_shape(shape(items=[agg("SUM", alias=None)]), A, B)
    assert not is_map_shape(shape(items=[agg("SUM", distinct=True)]), A, B)
    assert not is_map_shape(shape(items=[agg("COUNT", distinct=True)]), A, B)
    assert not is_map_shape(shape(items=[agg("STRING_AGG")]), A, B)
    assert not is_map_shape(shape(items=[SelItem(col("a", "name"))]), A, B)                 # none
    assert is_map_shape(shape(items=[agg("MAX", alias=f"x{i}") for i in range(8)]), A, B)
    assert not is_map_shape(shape(items=[agg("MAX", alias=f"x{i}") for i in range(9)]), A, B)
    assert not is_map_shape(shape(items=[agg("SUM"), SelItem(None, "e", expr=("lit", 1))]), A, B)
    # count_overlaps keeps the lone COUNT(b.col) under a bare LEFT ... ON
    assert not is_map_shape(shape(kind="LEFT", items=[agg("COUNT")]), A, B)
    assert is_map_shape(shape(kind="LEFT", items=[agg("COUNT")], on_terms=[SPATIAL, RESIDUAL]), A, B)
    assert is_map_shape(shape(kind="LEFT", items=[agg("COUNT"), agg("AVG", alias="m")]), A, B)
    assert is_map_shape(shape(kind="LEFT", items=[agg("COUNT", None)]), A, B)
    assert is_map_shape(shape(kind="INNER", items=[agg("COUNT")]), A, B)
    assert map_aggregate_ok("COUNT", "*", False) and not map_aggregate_ok("COUNT", "l", False)
    assert not map_aggregate_ok("MIN", "*", False) and not map_aggregate_ok("MIN", "r", True)


# ---------------------------------------------------------------- ... and on the plan, in execute()
def _plan(name="left_count_avg_max", **kw):
    return build_plan(Q.MAP_SHAPE[name], Q.TABLES, join_aggregates=True, **kw)


NUMERIC = {"score": pa.float64(), "weight": pa.int32(), "name": pa.string()}


def test_execute_routes_a_marked_plan_on_types_indices_and_devices():
    route = X._routes_join_aggregates
    plan = _plan()
    assert plan.join_aggregates and route(plan, NUMERIC, False, None)
    assert route(plan, NUMERIC, False, [0]) and not route(plan, NUMERIC, False, [0, 1])
    assert not route(plan, NUMERIC, True, None)                                   # return_indices
    assert not route(replace(plan, join_aggregates=False), NUMERIC, False, None)
    for t in (pa.int8(), pa.int16(), pa.int32(), pa.int64(), pa.float32(), pa.float64()):
        assert route(plan, dict(NUMERIC, score=t), False, None), t
    for t in (pa.string(), pa.large_string(), pa.bool_(), pa.uint32(), pa.float16(), pa.date32(), None):
        assert not route(plan, dict(NUMERIC, score=t), False, None), t            # MAX / AVG of such a column
    # COUNT takes a column of any type
    tail = _plan("inner_chrom_key")
    assert route(tail, NUMERIC, False, None) and not route(tail, dict(NUMERIC, name=None), False, None)
    lone = _plan("left_lone_count_with_residual")
    assert route(lone, {"name": pa.string()}, False, None)
    # a LEFT plan whose residuals are not all ON residuals, a projected right column: not the shape
    where = replace(lone, residuals=tuple(replace(r, clause="where") for r in lone.residuals))
    assert not route(where, {"name": pa.string()}, False, None)
    assert route(replace(where, kind="INNER"), {"name": pa.string()}, False, None)
    assert not route(replace(plan, projection=plan.projection + (X.Projection("r", "name", "chrom"),)), NUMERIC, False, None)


def test_aggregated_types_reads_arrow_and_numpy_tables():
    plan = _plan("eight_aggregates")
    rt = pa.table({"score": pa.array([1.0], pa.float32()), "weight": pa.array([1], pa.int16()),
                   "name": pa.array(["x"]).dictionary_encode()})
    assert X._aggregated_types(plan, rt) == {"name": pa.string(), "score": pa.float32(), "weight": pa.int16()}
    got = X._aggregated_types(plan, {"score": np.zeros(2), "weight": np.zeros(2, np.int64), "name": np.array(["x", "y"], object)})
    assert got["score"] == pa.float64() and got["weight"] == pa.int64() and not pa.types.is_floating(got["name"])


# ---------------------------------------------------------------- flag off: exactly the parent commit
ALL = {**Q.MAP_SHAPE, **Q.OUTSIDE}


def test_the_fixture_holds_exactly_the_queries_of_the_list():
    assert sorted(RECORDED["cases"]) == sorted(ALL) and len(RECORDED["recorded_at_commit"]) == 40
    assert len(ALL) == len(Q.MAP_SHAPE) + len(Q.OUTSIDE)
    for rec in RECORDED["cases"].values():
        assert sorted(rec) == sorted(Q.OPTIONS)
    assert "join_aggregates" not in json.dumps(RECORDED)


@pytest.mark.parametrize("name", sorted(ALL))
@pytest.mark.parametrize("opt", sorted(Q.OPTIONS))
def test_without_the_flag_every_query_lowers_as_recorded(name, opt):
    want = RECORDED["cases"][name][opt]
    assert Q.outcome(build_plan, ALL[name], **Q.OPTIONS[opt]) == want
    assert Q.outcome(build_plan, ALL[name], join_aggregates=False, **Q.OPTIONS[opt]) == want
    if "plan" in want:      # byte-identical plan strings, and the same plan object
        assert transpile(ALL[name], Q.TABLES, dialect="hip", **Q.OPTIONS[opt]) == want["plan"]
        assert build_plan(ALL[name], Q.TABLES, **Q.OPTIONS[opt]) == JoinPlan.from_string(want["plan"])
        assert not JoinPlan.from_string(want["plan"]).join_aggregates


# ---------------------------------------------------------------- flag on
@pytest.mark.parametrize("name", sorted(Q.OUTSIDE))
@pytest.mark.parametrize("opt", sorted(Q.OPTIONS))
def test_outside_the_shape_the_flag_changes_nothing(name, opt):
    assert Q.outcome(build_plan, Q.OUTSIDE[name], join_aggregates=True, **Q.OPTIONS[opt]) == RECORDED["cases"][name][opt]


@pytest.mark.parametrize("name", sorted(Q.MAP_SHAPE))
@pytest.mark.parametrize("opt", sorted(Q.OPTIONS))
def test_in_the_shape_the_plan_is_marked_and_is_otherwise_the_grouped_plan(name, opt):
    plan = build_plan(Q.MAP_SHAPE[name], Q.TABLES, join_aggregates=True, **Q.OPTIONS[opt])
    assert plan.join_aggregates and plan.kind in ("INNER", "LEFT") and plan.group_by
    assert 1 <= len(plan.aggregates) <= 8 and all(a.side in ("r", "*") for a in plan.aggregates)
    assert all(p.side == "l" and p.name in plan.group_by for p in plan.projection)
    assert plan.kind == ("LEFT" if name.startswith("left") else "INNER")
    assert plan == build_plan(Q.MAP_SHAPE[name], Q.TABLES, join_aggregates=True)        # (needs no outer_joins)
    want = RECORDED["cases"][name][opt]
    if "plan" in want:      # the plan of the parent commit, marked
        assert replace(plan, join_aggregates=False) == JoinPlan.from_string(want["plan"])
    else:                   # what declined: a COUNT beside other aggregates or residuals, a LEFT join without outer_joins
        assert want["error"] == "HipDeclined" and plan.kind == "LEFT"


def test_the_count_and_avg_left_query_plans():
    """The map recipe: declines without the flag, lowers to a LEFT plan with it -- without ``outer_joins``."""
    q = Q.MAP_SHAPE["left_count_avg_max"]
    assert "aggregate other than COUNT" in RECORDED["cases"]["left_count_avg_max"]["plain"]["message"]
    plan = build_plan(q, Q.TABLES, join_aggregates=True)
    assert (plan.kind, plan.predicate, plan.residuals, plan.join_aggregates) == ("LEFT", "intersects", (), True)
    assert [(a.func, a.side, a.column, a.name) for a in plan.aggregates] == [
        ("AVG", "r", "score", "mean"), ("COUNT", "r", "score", "n"), ("MAX", "r", "score", "mx")]
    assert plan.group_by == ("chrom", "start", "end") and plan.output == ("chrom", "start", "end", "mean", "n", "mx")


def test_a_lone_count_stays_the_count_plan():
    q = Q.OUTSIDE["lone_count_bare_on"]
    plan = build_plan(q, Q.TABLES, join_aggregates=True)
    assert plan.kind == "COUNT" and not plan.join_aggregates and plan == build_plan(q, Q.TABLES)


@pytest.mark.parametrize("name", sorted(Q.MAP_SHAPE))
def test_the_text_form_round_trips(name):
    q = Q.MAP_SHAPE[name]
    text = transpile(q, Q.TABLES, dialect="hip", join_aggregates=True)
    plan = JoinPlan.from_string(text)
    assert plan == build_plan(q, Q.TABLES, join_aggregates=True) and plan.join_aggregates
    assert plan.to_string() == text and '"join_aggregates":true' in text
    # an unmarked plan's string does not name the field at all: strings written before it existed are the strings of today
    assert "join_aggregates" not in replace(plan, join_aggregates=False).to_string()
    assert not JoinPlan.from_string(replace(plan, join_aggregates=False).to_string()).join_aggregates


def test_a_mark_needs_a_grouped_pair_plan():
    plan = _plan()
    for bad in (dict(kind="SEMI"), dict(aggregates=()), dict(group_by=())):
        with pytest.raises(ValueError, match="join_aggregates marks"):
            replace(plan, **bad)


def test_the_flag_reaches_every_entry_point():
    for fn in (build_plan, transpile, X.execute):
        p = inspect.signature(fn).parameters["join_aggregates"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY


def test_an_integer_sum_that_could_overflow_refuses():
    big = pa.array([2**40, -(2**41), None], pa.int64())
    X._check_int_sum("weight", big, 2**21, "pairs")                # 2^62: fits
    with pytest.raises(ValueError, match=r"SUM / AVG over column 'weight': 4194304 pairs .* can overflow the int64 sum"):
        X._check_int_sum("weight", big, 2**22, "pairs")            # 2^63: could wrap
    X._check_int_sum("weight", pa.array([None, None], pa.int64()), 2**62, "pairs")
    X._check_int_sum("weight", pa.array([0, 0], pa.int8()), 2**62, "pairs")


# ---------------------------------------------------------------- the C ABI
def test_the_header_s_symbols_are_the_binding_s():
    header = open(os.path.join(ROOT, "include", "giql_hip_pair_agg.h")).read()
    declared = sorted(set(re.findall(r"\b(giql_hip_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))))
    assert declared == sorted(_lib.PAIR_AGG_SYMBOLS)
    assert not set(_lib.PAIR_AGG_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.STRING_AGG_SYMBOLS) | set(_lib.RANGE_SET_SYMBOLS))
    assert re.search(r"#define GIQL_PAIR_AGG_MAX\s+8\b", header)
    main = open(os.path.join(ROOT, "include", "giql_hip.h")).read()
    assert "#define GIQL_HIP_ABI_VERSION 4 " in main and "giql_hip_pair_agg_dev" not in main
    L = _lib.load()
    assert L.giql_hip_abi_version() == 4
    assert all(hasattr(L, name) for name in _lib.PAIR_AGG_SYMBOLS)
    assert len(L.giql_hip_pair_agg_dev.argtypes) == 10
    # refused before any device is touched
    assert L.giql_hip_pair_agg_dev(None, None, None, 0, 0, 0, None, 0, None, None) == _lib.GIQL_ERR_INVALID


# ---------------------------------------------------------------- the reference against the sqlite-minted rows
def _golden_tables():
    cols = GOLDEN["columns"]
    return ({c: [r[i] for r in GOLDEN[t]] for i, c in enumerate(cols)} for t in ("a", "b"))


def _pairs(a, b, strand):
    return [(i, j) for i in range(len(a["chrom"])) for j in range(len(b["chrom"]))
            if a["chrom"][i] == b["chrom"][j] and a["start"][i] < b["end"][j] and b["start"][j] < a["end"][i]
            and (not strand or a["strand"][i] == b["strand"][j])]


@pytest.mark.parametrize("case", [c for c in GOLDEN["cases"] if c["keys"] == ["chrom", "start", "end"]],
                         ids=lambda c: c["name"])
def test_the_reference_answers_the_golden_rows(case):
    """Grouped by the (distinct) left interval a group is one left row: the per-row reference IS the query."""
    a, b = _golden_tables()
    pairs = _pairs(a, b, case["strand"])
    aggs = [(f, c) for f, c in GOLDEN["aggregates"] if c != "*"]
    n_pairs, res = R.pair_aggregate([p[0] for p in pairs], [p[1] for p in pairs], len(a["chrom"]), b, aggs)
    rows = []
    for i in range(len(a["chrom"])):
        if case["join"] == "INNER" and not n_pairs[i]:
            continue
        it = iter(r[i] for r in res)
        rows.append([a["chrom"][i], a["start"][i], a["end"][i]]
                    + [max(n_pairs[i], 1) if c == "*" else next(it) for _f, c in GOLDEN["aggregates"]])
    assert sorted(rows, key=lambda r: r[:3]) == case["rows"]


def test_the_reference_reduces_in_ascending_right_row_whatever_the_order_of_the_pairs():
    row_a, row_b = [2, 0, 2, 2, 0], [5, 1, 0, 5, 3]
    assert R.members(row_a, row_b, 4) == [[1, 3], [], [0, 5, 5], []]
    cols = {"v": [1.5, None, 0.0, float("nan"), 9.0, -2.0]}
    pairs, (s, mn, mx, n, avg) = R.pair_aggregate(row_a, row_b, 4, cols, [(f, "v") for f in ("SUM", "MIN", "MAX", "COUNT", "AVG")])
    assert pairs == [2, 0, 3, 0] and n == [1, 0, 3, 0]
    assert s[0] != s[0] and mn[0] != mn[0] and mx[0] != mx[0]       # NaN alone: NaN
    assert (s[1], mn[1], mx[1], avg[1]) == (None, None, None, None)
    assert (s[2], mn[2], mx[2], avg[2]) == (-2.5, -2.0, 1.5, -2.5 / 3)


# ---------------------------------------------------------------- the host combine of the per-row partials
COMBINE = ("SELECT a.name, AVG(b.weight) AS m, SUM(b.weight) AS s, MIN(b.score) AS lo, MAX(b.score) AS hi, "
           "COUNT(*) AS c, COUNT(b.score) AS n FROM a {join} JOIN b ON a.interval INTERSECTS b.interval GROUP BY a.name")


def _combine(join, names, pairs, weight, score):
    """``weight`` / ``score``: per left row ``(value, non-NULL count)``; MIN and MAX share the ``score`` values."""
    plan = build_plan(COMBINE.format(join=join), Q.TABLES, join_aggregates=True)
    w = (np.array([v for v, _n in weight], np.int64), np.array([n for _v, n in weight], np.int64))
    s = (np.array([v for v, _n in score], np.float64), np.array([n for _v, n in score], np.int64))
    out = X._combine_join_partials(plan, {"name": np.array(names, object)}, np.array(pairs, np.int64),
                                   {("SUM", "weight"): w, ("MIN", "score"): s, ("MAX", "score"): s, ("COUNT", "score"): s},
                                   {"weight": pa.int64(), "score": pa.float64()})
    return {r["name"]: r for r in out.to_pylist()}


def test_an_integer_avg_past_2_pow_53_is_the_rounded_quotient_not_an_error():
    """Per-key sums between 2^53 and 2^63 pass the overflow guard: AVG is ``float(sum) / count``, as without the flag."""
    big = 2**53 + 1          # (not a double)
    got = _combine("INNER", ["x", "x", "y", "z"], [3, 2, 1, 1],
                   [(big, 3), (2**60 + 7, 2), (-(2**62) - 3, 1), (5, 1)], [(0.0, 0)] * 4)
    assert got["x"]["s"] == big + 2**60 + 7 and got["x"]["m"] == float(big + 2**60 + 7) / 5
    assert got["y"]["s"] == -(2**62) - 3 and got["y"]["m"] == float(-(2**62) - 3)
    assert (got["z"]["s"], got["z"]["m"]) == (5, 5.0)
    # ... which is what the path without the flag answers: pyarrow's mean over the key's five pair values
    import pyarrow.compute as pc

    per_pair = pa.array([2**52, 2**52, 1, 2**59, 2**59 + 7], pa.int64())
    assert sum(per_pair.to_pylist()) == got["x"]["s"] and pc.mean(per_pair).as_py() == got["x"]["m"]


def test_float_min_max_keep_the_nan_order_across_the_rows_of_a_key():
    nan = float("nan")
    # per left row: (the device's MIN or MAX, non-NULL inputs) -- one call per function, the rows' values differ
    rows = ["k1", "k1", "k2", "k2", "k3", "k3", "k4", "k5", "k5"]
    pairs = [2, 1, 1, 1, 1, 2, 1, 0, 0]
    none = [(0, 0)] * len(rows)
    # as MIN: a row's NaN means "only NaNs there"
    mins = [(1.5, 2), (nan, 1), (nan, 1), (nan, 1), (0.0, 0), (-2.0, 1), (0.0, 0), (0.0, 0), (0.0, 0)]
    lo = {k: r["lo"] for k, r in _combine("LEFT", rows, pairs, none, mins).items()}
    assert lo["k1"] == 1.5 and lo["k2"] != lo["k2"] and lo["k3"] == -2.0 and lo["k4"] is None and lo["k5"] is None
    # as MAX: a row's NaN means "a NaN among its inputs"
    maxs = [(1.5, 2), (nan, 1), (nan, 1), (nan, 1), (0.0, 0), (-2.0, 1), (0.0, 0), (0.0, 0), (0.0, 0)]
    res = _combine("LEFT", rows, pairs, none, maxs)
    hi = {k: r["hi"] for k, r in res.items()}
    assert hi["k1"] != hi["k1"] and hi["k2"] != hi["k2"] and hi["k3"] == -2.0 and hi["k4"] is None and hi["k5"] is None
    # LEFT: COUNT(*) counts one padded row per unmatched left row, COUNT(col) none
    assert (res["k5"]["c"], res["k5"]["n"], res["k4"]["c"], res["k1"]["c"], res["k1"]["n"]) == (2, 0, 1, 3, 3)
    inner = _combine("INNER", rows, pairs, none, maxs)
    assert sorted(inner) == ["k1", "k2", "k3", "k4"] and inner["k4"]["hi"] is None
