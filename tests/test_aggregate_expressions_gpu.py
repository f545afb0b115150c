"""``execute(..., join_aggregates=True, aggregate_expressions=True)`` on the GPU: aggregates over an expression of a
join's pair in the map shape ("Overlap Statistics", docs/recipes/advanced.rst), against the sqlite-minted rows of
tests/golden/aggregate_expressions.json and against the only route the same numbers had before: the per-pair output
of ``select_expressions=True`` grouped on the host with pyarrow.

Exactness: everything compares with ``==``.  The tables hold integers, and scores that are multiples of 1/4 with
weights that are 0 or plus / minus a power of two: every per-pair value is a multiple of 1/16 far below 2^53, so every
sum is exact in binary64 in any order and a mean is one division of exact numbers on both sides."""
import json
import os

import numpy as np
import pytest

import _pair_expr_agg_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
pa = pytest.importorskip("pyarrow")
pc = pytest.importorskip("pyarrow.compute")

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "aggregate_expressions.json")))
T = ["a", "b"]
ON = "a.interval INTERSECTS b.interval"
BOTH = {"join_aggregates": True, "aggregate_expressions": True}
TYPES = {"chrom": pa.string(), "start": pa.int32(), "end": pa.int32(), "name": pa.string(), "score": pa.float64(),
         "weight": pa.int32()}


@pytest.fixture(scope="module")
def eng():
    from giql_amd.engine import HipEngine

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    e = HipEngine(0)
    yield e
    e.close()


def _arrow(t):
    return pa.table({k: pa.array(v, TYPES[k]) for k, v in t.items()})


@pytest.fixture(scope="module")
def golden():
    a, b = R.golden_tables(GOLDEN)
    return a, b, _arrow(a), _arrow(b)


def _sort_key(n_keys):
    return lambda r: [(x is not None, x) for x in r[:n_keys]]


def _rows(tbl, names):
    return [list(r) for r in zip(*(tbl.column(c).to_pylist() for c in names))]


# ---------------------------------------------------------------- the sqlite-minted rows
@pytest.mark.parametrize("case", GOLDEN["cases"], ids=lambda c: c["name"])
def test_the_golden_rows(eng, golden, case):
    """One query per expression (COUNT(*) and the five functions of it: six of the eight aggregates a plan takes)."""
    from giql_amd.execute import execute

    _a, _b, ta, tb = golden
    keys = ", ".join(f"a.{k}" for k in case["keys"])
    funcs, n_keys = GOLDEN["functions"], len(case["keys"])
    for j, (name, text) in enumerate(GOLDEN["expressions"].items()):
        aggs = ", ".join(f"{f}({text}) AS {f.lower()}_{name}" for f in funcs)
        out = execute(f"SELECT {keys}, COUNT(*) AS n, {aggs} FROM a {case['join']} JOIN b ON {ON} GROUP BY {keys}",
                      {"a": ta, "b": tb}, eng, giql_tables=T, **BOTH)
        got = _rows(out, case["keys"] + ["n"] + [f"{f.lower()}_{name}" for f in funcs])
        lo = n_keys + 1 + j * len(funcs)
        want = [r[:n_keys + 1] + r[lo:lo + len(funcs)] for r in case["rows"]]
        assert sorted(got, key=_sort_key(n_keys)) == sorted(want, key=_sort_key(n_keys)), name
        # SUM / MIN / MAX come back as int64 or float64 by the rule of the computed columns
        flt = name in ("weighted", "ratio")
        assert out.schema.field(f"sum_{name}").type == (pa.float64() if flt else pa.int64())
        assert out.schema.field(f"max_{name}").type == (pa.float64() if flt else pa.int64())
        assert out.schema.field(f"avg_{name}").type == pa.float64() and out.schema.field(f"count_{name}").type == pa.int64()


def test_the_overlap_statistics_recipe_and_its_left_per_peak_variant(eng, golden):
    from giql_amd.execute import execute

    a, b, ta, tb = golden
    ov = GOLDEN["expressions"]["overlap_bp"]
    out = execute(f"SELECT a.chrom, COUNT(*) AS overlap_count, AVG({ov}) AS avg_overlap_bp, SUM({ov}) AS total_overlap_bp "
                  f"FROM a INNER JOIN b ON {ON} GROUP BY a.chrom ORDER BY a.chrom", {"a": ta, "b": tb}, eng, giql_tables=T, **BOTH)
    rows = next(c for c in GOLDEN["cases"] if c["name"] == "inner_chrom")["rows"]
    assert _rows(out, ["chrom", "overlap_count", "avg_overlap_bp", "total_overlap_bp"]) == [[r[0], r[1], r[4], r[3]] for r in rows]
    case = GOLDEN["expressions"]["overlap_case"]
    out = execute(f"SELECT a.chrom, a.start, a.end, SUM({ov}) AS bp, SUM({case}) AS covered, SUM(b.end - a.start) AS reach "
                  f"FROM a LEFT JOIN b ON {ON} GROUP BY a.chrom, a.start, a.end ORDER BY a.chrom, a.start, a.end",
                  {"a": ta, "b": tb}, eng, giql_tables=T, **BOTH)
    rows = next(c for c in GOLDEN["cases"] if c["name"] == "left_interval")["rows"]
    n = len(GOLDEN["functions"])
    assert _rows(out, ["chrom", "start", "end", "bp", "covered", "reach"]) == \
        [r[:3] + [r[5], r[5 + n], r[5 + 3 * n]] for r in rows]
    unmatched = [g for g, r in zip(_rows(out, ["start", "end", "bp", "covered", "reach"]), rows) if r[3] == 1 and r[4 + 3 * n] == 0]
    assert unmatched and all(g[2] == g[1] - g[0] and g[3] == 0 and g[4] is None for g in unmatched)


def test_having_order_by_and_limit_on_an_aliased_aggregate(eng, golden):
    from giql_amd.execute import execute

    _a, _b, ta, tb = golden
    ov = GOLDEN["expressions"]["overlap_bp"]
    for join in ("INNER", "LEFT"):
        rows = next(c for c in GOLDEN["cases"] if c["name"] == f"{join.lower()}_interval")["rows"]
        kept = sorted((r for r in rows if r[5] > 40), key=lambda r: (-r[5], r[0], r[1], r[2]))[:7]
        out = execute(f"SELECT a.chrom, a.start, a.end, SUM({ov}) AS bp, MAX({ov}) AS widest FROM a {join} JOIN b ON {ON} "
                      "GROUP BY a.chrom, a.start, a.end HAVING bp > 40 ORDER BY bp DESC, a.chrom, a.start, a.end LIMIT 7",
                      {"a": ta, "b": tb}, eng, giql_tables=T, **BOTH)
        assert _rows(out, ["chrom", "start", "end", "bp", "widest"]) == [r[:3] + [r[5], r[8]] for r in kept], join


def test_a_pinned_table_s_index_serves_the_pairs(eng, golden):
    from giql_amd.execute import execute, pin

    _a, _b, ta, tb = golden
    text = GOLDEN["expressions"]["weighted"]
    n = len(GOLDEN["functions"])
    with pin(tb, index=True) as pb:
        for join in ("INNER", "LEFT"):
            out = execute(f"SELECT a.name, SUM({text}) AS w, COUNT({text}) AS k FROM a {join} JOIN b ON {ON} GROUP BY a.name",
                          {"a": ta, "b": pb}, eng, giql_tables=T, **BOTH)
            rows = next(c for c in GOLDEN["cases"] if c["name"] == f"{join.lower()}_name")["rows"]
            want = [[r[0], r[2 + 2 * n + 1], r[2 + 2 * n]] for r in rows]
            assert sorted(_rows(out, ["name", "w", "k"]), key=_sort_key(1)) == sorted(want, key=_sort_key(1)), join


def test_an_integer_sum_that_could_overflow_refuses_and_a_float_tree_is_exempt(eng):
    from giql_amd.execute import execute

    big = 2**31
    ta = pa.table({"chrom": ["c"] * 2, "start": pa.array([0, 10], pa.int32()), "end": pa.array([100, 90], pa.int32()),
                   "v": pa.array([big, -big], pa.int64())})
    tb = pa.table({"chrom": ["c"] * 3, "start": pa.array([5, 20, 30], pa.int32()), "end": pa.array([50, 60, 70], pa.int32()),
                   "v": pa.array([big, big, 3], pa.int64())})
    q = "SELECT a.chrom, {agg} AS total FROM a JOIN b ON a.interval INTERSECTS b.interval GROUP BY a.chrom"
    with pytest.raises(ValueError, match=r"aggregate 'total': 6 values of magnitude up to 4611686018427387904 can overflow"):
        execute(q.format(agg="SUM(a.v * b.v)"), {"a": ta, "b": tb}, eng, giql_tables=T, **BOTH)
    with pytest.raises(ValueError, match="aggregate 'total'"):
        execute(q.format(agg="AVG(a.v * b.v)"), {"a": ta, "b": tb}, eng, giql_tables=T, **BOTH)
    out = execute(q.format(agg="SUM(a.v * b.v * 1.0)"), {"a": ta, "b": tb}, eng, giql_tables=T, **BOTH)
    assert out.column("total").to_pylist() == [0.0] and out.schema.field("total").type == pa.float64()
    out = execute(q.format(agg="MAX(a.v * b.v)"), {"a": ta, "b": tb}, eng, giql_tables=T, **BOTH)     # no sum: no bound
    assert out.column("total").to_pylist() == [2**62]
    out = execute(q.format(agg="SUM(a.v + b.v)"), {"a": ta, "b": tb}, eng, giql_tables=T, **BOTH)
    assert out.column("total").to_pylist() == [(big + big) * 2 + (big + 3) + (-big + big) * 2 + (-big + 3)]


# ---------------------------------------------------------------- against the per-pair route grouped on the host
def _table(r, n, names, span=30_000, chroms=("chr1", "chr2", "chr3")):
    start = r.integers(0, span, n)
    score = (r.integers(-800, 800, n) / 4.0).tolist()
    weight = r.choice([0, 1, 2, 4, -1, -2], n).tolist()
    name = r.choice(names, n).tolist()
    for col, p in ((score, 0.3), (weight, 0.2), (name, 0.1)):
        for i in np.nonzero(r.random(n) < p)[0]:
            col[i] = None
    return {"chrom": r.choice(chroms, n).tolist(), "start": start.tolist(), "end": (start + r.integers(1, 600, n)).tolist(),
            "name": name, "score": score, "weight": weight}


@pytest.mark.parametrize("join", ["INNER", "LEFT"])
def test_equal_to_grouping_the_per_pair_output_on_the_host(eng, join):
    """The only route these numbers had before: ``select_expressions=True`` projects the key and the expression per
    pair (per padded row under LEFT, with ``outer_joins``), pyarrow groups.  Several tiles of pairs, keys that repeat."""
    from giql_amd.execute import execute

    r = np.random.default_rng(77)
    a, b = _table(r, 400, ["g%d" % i for i in range(9)]), _table(r, 900, ["x"])
    a["chrom"][:4] = ["chrQ"] * 4                       # unmatched left rows
    tables = {"a": _arrow(a), "b": _arrow(b)}
    exprs = {"bp": GOLDEN["expressions"]["overlap_bp"], "cs": GOLDEN["expressions"]["overlap_case"],
             "w": GOLDEN["expressions"]["weighted"], "q": GOLDEN["expressions"]["ratio"], "d": "ABS(a.score - b.score)"}
    per_pair = execute("SELECT a.name, " + ", ".join(f"{t} AS {n}" for n, t in exprs.items()) + f" FROM a {join} JOIN b ON {ON}",
                       tables, eng, giql_tables=T, select_expressions=True, outer_joins=True)
    assert per_pair.num_rows > 4 * 256
    for group in (("bp", "cs"), ("w", "q"), ("d",)):       # at most eight aggregates a query
        fns = ("sum", "min", "max", "count") if len(group) == 2 else ("sum", "min", "max", "count", "mean")
        host = per_pair.group_by(["name"], use_threads=False).aggregate([(n, f) for n in group for f in fns])
        sql = {"sum": "SUM", "min": "MIN", "max": "MAX", "count": "COUNT", "mean": "AVG"}
        aggs = ", ".join(f"{sql[f]}({exprs[n]}) AS {n}_{f}" for n in group for f in fns)
        out = execute(f"SELECT a.name, {aggs} FROM a {join} JOIN b ON {ON} GROUP BY a.name", tables, eng, giql_tables=T, **BOTH)
        names = ["name"] + [f"{n}_{f}" for n in group for f in fns]
        assert sorted(_rows(out, names), key=_sort_key(1)) == sorted(_rows(host, names), key=_sort_key(1)), group
