"""Aggregates beside MERGE (``merge_aggregates=True``): the plan builder, the declines and loud errors, the overflow
guard, the plain-Python reference against the sqlite-minted rows, and the C ABI's declaration.  The GPU half is
tests/test_merge_aggregates_gpu.py."""
import json
import os

import pytest

import _merge_agg_ref as R
from giql_amd.plan import Aggregate, JoinPlan, Projection
from giql_amd.transpile import HipDeclined, build_plan, transpile

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "merge_aggregates.json")))

# docs/recipes/bedtools-migration.rst "-c -o mean"; docs/recipes/clustering.rst "Merge with Aggregations"
RECIPES = [
    ("SELECT MERGE(interval), AVG(score) AS avg_score FROM features",
     [("agg", "0", "avg_score")], [("AVG", "score", "avg_score")], 0),
    ("SELECT MERGE(interval), COUNT(*) AS feature_count, AVG(score) AS avg_score, MAX(score) AS max_score, "
     "SUM(score) AS total_score FROM features",
     [("count", "*", "feature_count"), ("agg", "0", "avg_score"), ("agg", "1", "max_score"), ("agg", "2", "total_score")],
     [("AVG", "score", "avg_score"), ("MAX", "score", "max_score"), ("SUM", "score", "total_score")], 0),
    ("SELECT MERGE(interval, 1000), COUNT(*) AS n, MAX(score) AS hi FROM features",
     [("count", "*", "n"), ("agg", "0", "hi")], [("MAX", "score", "hi")], 1000),
    ("SELECT MERGE(interval, stranded := true), MIN(f.weight) AS lo, COUNT(weight) AS k, COUNT(*) AS n FROM features f",
     [("agg", "0", "lo"), ("agg", "1", "k"), ("count", "*", "n")], [("MIN", "weight", "lo"), ("COUNT", "weight", "k")], 0),
]


@pytest.mark.parametrize("query, projection, aggregates, distance", RECIPES)
def test_recipes_lower_to_a_merge_plan_with_the_aggregates_in_select_order(query, projection, aggregates, distance):
    plan = build_plan(query, ["features"], merge_aggregates=True)
    assert plan.kind == "MERGE" and plan.distance == distance
    assert plan.projection == tuple(Projection(*p) for p in projection)
    assert plan.aggregates == tuple(Aggregate(f, "l", c, name) for f, c, name in aggregates)
    text = transpile(query, ["features"], dialect="hip", merge_aggregates=True)
    assert text == plan.to_string() and JoinPlan.from_string(text) == plan
    assert JoinPlan.from_string(text).to_string() == text


@pytest.mark.parametrize("query", [r[0] for r in RECIPES])
def test_without_the_keyword_the_same_texts_decline_as_before(query):
    with pytest.raises(HipDeclined, match="function call in the SELECT list|aggregate other than COUNT"):
        build_plan(query, ["features"])
    with pytest.raises(HipDeclined):
        transpile(query, ["features"], dialect="hip")


def test_a_plan_without_aggregates_keeps_its_string():
    q = "SELECT MERGE(interval, 10), COUNT(*) AS n FROM features"
    assert transpile(q, ["features"], dialect="hip", merge_aggregates=True) == transpile(q, ["features"], dialect="hip")
    assert '"aggregates":[]' in transpile(q, ["features"], dialect="hip")


@pytest.mark.parametrize("query, message", [
    ("SELECT MERGE(interval), SUM(score) FROM features", "without an alias beside MERGE"),
    ("SELECT MERGE(interval), SUM(DISTINCT score) AS s FROM features", "DISTINCT inside SUM"),
    ("SELECT MERGE(interval), COUNT(DISTINCT score) AS s FROM features", "DISTINCT inside COUNT"),
    ("SELECT MERGE(interval), SUM(score * 2) AS s FROM features", "expression argument of SUM"),
    ("SELECT MERGE(interval), MAX(ABS(score)) AS s FROM features", "expression argument of MAX"),
    ("SELECT MERGE(interval), STRING_AGG(name, ',') AS names FROM features", "STRING_AGG beside MERGE"),
    ("SELECT *, CLUSTER(interval) AS cid, SUM(score) AS s FROM features", "aggregate beside CLUSTER"),
    ("SELECT *, CLUSTER(interval) AS cid, COUNT(score) AS s FROM features", "aggregate beside CLUSTER"),
    ("SELECT MERGE(interval), " + ", ".join(f"SUM(c{k}) AS s{k}" for k in range(9)) + " FROM features",
     "more than 8 aggregates"),
])
def test_what_still_declines_says_so(query, message):
    with pytest.raises(HipDeclined, match=message):
        build_plan(query, ["features"], merge_aggregates=True)


@pytest.mark.parametrize("query, message", [
    ("SELECT MERGE(interval), SUM(score) AS start FROM features", "collides with chrom/start/end"),
    ("SELECT MERGE(interval), AVG(score) AS chrom FROM features", "collides with chrom/start/end"),
    ("SELECT MERGE(interval), SUM(score) AS s, MAX(score) AS s FROM features", "collides with chrom/start/end"),
    ("SELECT MERGE(interval), score, SUM(score) AS s FROM features", "non-aggregated column 'score'"),
    ("SELECT MERGE(interval), SUM(g.score) AS s FROM features f", "Unknown table qualifier"),
])
def test_the_reference_s_loud_errors_stay_value_errors(query, message):
    with pytest.raises(ValueError, match=message) as exc:
        build_plan(query, ["features"], merge_aggregates=True)
    assert not isinstance(exc.value, HipDeclined)


def test_eight_aggregates_lower_and_the_projection_must_name_one():
    q = "SELECT MERGE(interval), " + ", ".join(f"SUM(c{k}) AS s{k}" for k in range(8)) + " FROM features"
    plan = build_plan(q, ["features"], merge_aggregates=True)
    assert [a.column for a in plan.aggregates] == [f"c{k}" for k in range(8)]
    with pytest.raises(ValueError, match="names aggregate"):
        JoinPlan("MERGE", plan.left, None, (Projection("agg", "1", "x"),), aggregates=plan.aggregates[:1])


def test_the_overflow_guard_trips_at_the_bound_and_not_below_it():
    pa = pytest.importorskip("pyarrow")
    from giql_amd.execute import _check_int_sum

    # 4 rows: 4 * 2^61 = 2^63 is refused, 4 * (2^61 - 1) < 2^63 passes; the magnitude counts, not the sign
    _check_int_sum("w", pa.array([2**61 - 1, 0, -5, None], pa.int64()))
    _check_int_sum("w", pa.array([-(2**61) + 1, 0, 7, 1], pa.int64()))
    for values in ([2**61, 0, 1, None], [3, -(2**61), 1, 1]):
        with pytest.raises(ValueError, match="column 'w'.*overflow"):
            _check_int_sum("w", pa.array(values, pa.int64()))
    _check_int_sum("w", pa.array([None, None], pa.int64()))
    # an int32 column reaches the bound only at 2^32 rows
    _check_int_sum("w", pa.array([-(2**31)] * 1000, pa.int32()))


def _sig(v):
    return float(f"{v:.12g}") if isinstance(v, float) else v


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=lambda c: c["name"])
def test_the_reference_reproduces_the_sqlite_minted_rows(case):
    rows = GOLDEN["rows"]
    part = [(r[0], r[3]) if case["stranded"] else (r[0],) for r in rows]
    columns = {"score": [r[4] for r in rows], "weight": [r[5] for r in rows]}
    got = R.merge_agg(part, [r[1] for r in rows], [r[2] for r in rows], case["distance"], columns,
                      [tuple(a) for a in GOLDEN["aggregates"]])
    k = len(part[0])
    got = sorted(([*r[0], *map(_sig, r[1:])] for r in got), key=lambda r: (r[0], r[k]))   # ORDER BY chrom, start
    want = sorted(([_sig(v) for v in r] for r in case["merged"]), key=lambda r: (r[0], r[k]))
    assert got == want


def test_the_two_oracle_restatements_give_the_reference_the_same_cluster_ids():
    import numpy as np
    from oracle import pyoracle as ora

    rows = GOLDEN["rows"]
    codes = {c: k for k, c in enumerate(sorted({r[0] for r in rows}))}
    side = ora.Side(np.array([codes[r[0]] for r in rows]), np.array([r[1] for r in rows]), np.array([r[2] for r in rows]))
    for distance in (0, 25):
        want = ora.py_cluster(side, distance).tolist()
        assert ora.c_cluster(side, distance).tolist() == want
        assert R.cluster_ids([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], distance) == want


def test_reference_nan_order_and_nulls():
    nan = float("nan")
    assert R.aggregate("MAX", [1.0, nan, 3.0]) != R.aggregate("MAX", [1.0, nan, 3.0])      # NaN
    assert R.aggregate("MIN", [1.0, nan, None, -3.0]) == -3.0
    assert R.aggregate("MIN", [nan, None, nan]) != R.aggregate("MIN", [nan, None, nan])
    assert R.aggregate("SUM", [1.0, nan]) != R.aggregate("SUM", [1.0, nan])
    assert R.aggregate("SUM", [None, None]) is None and R.aggregate("COUNT", [None, None]) == 0
    assert R.aggregate("AVG", [1, 2, None]) == 1.5 and R.aggregate("SUM", [2**62, 2**62, 2**62]) == 3 * 2**62


def test_the_header_declares_the_call_and_the_binding_lists_it():
    from giql_amd import _lib

    header = open(os.path.join(HERE, "..", "include", "giql_hip.h")).read()
    assert "int giql_hip_merge_agg_dev(giql_hip_ctx* ctx, const giql_side* s" in header
    assert "typedef struct giql_agg {" in header
    assert "enum { GIQL_AGG_COUNT = 0" in header and "GIQL_AGG_MAX = 3 }" in header
    assert "#define GIQL_HIP_ABI_VERSION 4 " in header
    assert "giql_hip_merge_agg_dev" in _lib.SYMBOLS
    assert _lib.AGG_FUNCS == {"COUNT": 0, "SUM": 1, "MIN": 2, "MAX": 3}
    assert [f[0] for f in _lib.CAgg._fields_] == ["func", "type", "data", "valid", "out", "out_nn"]


def test_the_built_library_exports_the_call():
    from giql_amd import _lib

    L = _lib.load()
    assert L.giql_hip_abi_version() == 4
    assert L.giql_hip_merge_agg_dev.argtypes is not None and len(L.giql_hip_merge_agg_dev.argtypes) == 15
