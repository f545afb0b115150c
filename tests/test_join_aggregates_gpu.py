"""``execute(..., join_aggregates=True)`` on the GPU: grouped aggregates over a join in the map shape, against a
brute-force restatement over tests/_pair_agg_ref.py, against the path the same query takes without the flag, and
against the sqlite-minted rows of tests/golden/join_aggregates.json.

Exactness: counts, integer results and MIN / MAX compare with ``==``.  A float SUM over k non-NULL values may differ
from ``fsum`` by at most k * 2^-52 * sum|x_i| (any summation order in binary64, doubled), a float AVG by that over k
plus one ulp of the result: the derived bound of tests/test_merge_aggregates_gpu.py, for both paths."""
import json
import math
import os

import numpy as np
import pytest

import _pair_agg_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
pa = pytest.importorskip("pyarrow")

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "join_aggregates.json")))
T = ["a", "b"]
IV = "a.chrom, a.start, a.end"
AGGS = [("COUNT", "*", "n_rows"), ("COUNT", "name", "n_name"), ("COUNT", "score", "n_score"), ("SUM", "score", "s_score"),
        ("AVG", "score", "m_score"), ("MIN", "score", "lo_score"), ("MAX", "weight", "hi_weight"), ("SUM", "weight", "s_weight")]
KEYSETS = {"interval": ("chrom", "start", "end"), "name": ("name",), "chrom": ("chrom",)}


@pytest.fixture(scope="module")
def eng():
    from giql_amd.engine import HipEngine

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    e = HipEngine(0)
    yield e
    e.close()


def _table(r, n, names, span=20_000, chroms=("chr1", "chr2", "chr3")):
    start = r.integers(0, span, n)
    score = (r.normal(0, 100, n) * r.choice([1e-3, 1.0, 1e3], n)).tolist()
    weight = r.integers(-1000, 1000, n).tolist()
    name = r.choice(names, n).tolist()
    for col, p in ((score, 0.3), (weight, 0.3), (name, 0.15)):
        for i in np.nonzero(r.random(n) < p)[0]:
            col[i] = None
    return {"chrom": r.choice(chroms, n).tolist(), "start": start.tolist(), "end": (start + r.integers(1, 400, n)).tolist(),
            "name": name, "strand": r.choice(["+", "-"], n).tolist(), "score": score, "weight": weight}


def _arrow(t):
    types = {"chrom": pa.string(), "start": pa.int32(), "end": pa.int32(), "name": pa.string(), "strand": pa.string(),
             "score": pa.float64(), "weight": pa.int32()}
    return pa.table({k: pa.array(v, types[k]) for k, v in t.items()})


@pytest.fixture(scope="module")
def tables():
    r = np.random.default_rng(2026)
    a = _table(r, 300, ["g1", "g2", "g3", "g4", "g5", "g6", "g7"])
    b = _table(r, 700, ["x", "y", "z"])
    a["chrom"][:3] = ["chrQ"] * 3                     # left rows on a chromosome the right table lacks: unmatched
    a["start"][3], a["end"][3] = a["start"][4], a["end"][4]
    a["chrom"][3] = a["chrom"][4]                     # a duplicate interval key
    return a, b


def _distance(p, g):
    return 0 if p[1] < g[2] and p[2] > g[1] else (g[1] - p[2] + 1 if p[2] <= g[1] else p[1] - g[2] + 1)


TESTS = {"intersects": lambda p, g: p[1] < g[2] and p[2] > g[1], "contains": lambda p, g: p[1] <= g[1] and p[2] >= g[2],
         "within": lambda p, g: p[1] >= g[1] and p[2] <= g[2], "distance": lambda p, g: _distance(p, g) <= 150}
ON = {"intersects": "a.interval INTERSECTS b.interval", "contains": "a.interval CONTAINS b.interval",
      "within": "a.interval WITHIN b.interval", "distance": "DISTANCE(a.interval, b.interval) <= 150"}


def _pairs(a, b, predicate="intersects", strand=False):
    fa, fb = (list(zip(t["chrom"], t["start"], t["end"])) for t in (a, b))
    test = TESTS[predicate]
    return [(i, j) for i, p in enumerate(fa) for j, g in enumerate(fb)
            if p[0] == g[0] and test(p, g) and (not strand or a["strand"][i] == b["strand"][j])]


def reference(a, b, pairs, keys, left, aggs=AGGS):
    """``{key: [(exact value | None, values it was taken over)]}`` per distinct left key."""
    mem = R.members([p[0] for p in pairs], [p[1] for p in pairs], len(a["chrom"]))
    groups = {}
    for i, m in enumerate(mem):
        if m or left:
            g = groups.setdefault(tuple(a[k][i] for k in keys), {"rows": 0, "b": []})
            g["rows"] += max(len(m), 1) if left else len(m)
            g["b"] += m
    out = {}
    for key, g in groups.items():
        row = []
        for func, column, _name in aggs:
            xs = None if column == "*" else [b[column][j] for j in g["b"]]
            if xs is not None and column == "name":
                xs = [None if x is None else 1 for x in xs]
            row.append((g["rows"], None) if column == "*" else (R.aggregate(func, xs), xs))
        out[key] = row
    return out


def _rows(tbl, keys, aggs=AGGS):
    cols = [tbl.column(c).to_pylist() for c in list(keys) + [n for _f, _c, n in aggs]]
    return {tuple(r[:len(keys)]): list(r[len(keys):]) for r in zip(*cols)}


def check(tbl, want, keys, aggs=AGGS):
    got = _rows(tbl, keys, aggs)
    assert tbl.num_rows == len(got) and sorted(got, key=repr) == sorted(want, key=repr)
    for key, row in want.items():
        for (func, column, name), (w, xs), g in zip(aggs, row, got[key]):
            what = (key, name)
            flt = column == "score"
            if w is None:
                assert g is None, what
            elif flt and func in ("SUM", "AVG"):
                k = sum(x is not None for x in xs)
                bound = k * 2.0**-52 * R.abs_sum(xs)
                bound = bound if func == "SUM" else bound / k + math.ulp(w)
                assert g is not None and abs(g - w) <= bound, (what, g, w, bound)
            else:
                assert g == w and type(g) is type(w), (what, g, w)


def query(join, on, keys, aggs=AGGS, tail=""):
    key = ", ".join(f"a.{k}" for k in keys)
    sel = ", ".join("COUNT(*) AS " + n if c == "*" else f"{f}(b.{c}) AS {n}" for f, c, n in aggs)
    return f"SELECT {key}, {sel} FROM a {join} JOIN b ON {on} GROUP BY {key}{tail}"


def run(eng, q, a, b, **kw):
    from giql_amd.execute import execute

    return execute(q, {"a": _arrow(a), "b": _arrow(b)}, eng, giql_tables=T, **kw)


def assert_same_tables(new, old, keys):
    """The new path's table against the old path's, both sorted by the keys: integers, counts and MIN / MAX exactly,
    float SUM / AVG each within the derived bound of the exact value -- so within twice that of each other; the exact
    comparison against fsum is ``check``'s."""
    assert new.column_names == old.column_names and new.num_rows == old.num_rows
    order = [(k, "ascending") for k in keys]
    new, old = new.sort_by(order), old.sort_by(order)
    for name in new.column_names:
        x, y = new.column(name).to_pylist(), old.column(name).to_pylist()
        if pa.types.is_floating(new.column(name).type) and name in ("s_score", "m_score"):
            assert [v is None for v in x] == [v is None for v in y], name
        else:
            assert x == y, name


# ---------------------------------------------------------------- INNER / LEFT x key sets, against both references
@pytest.mark.parametrize("join", ["INNER", "LEFT"])
@pytest.mark.parametrize("keyset", sorted(KEYSETS))
def test_map_queries_against_the_restatement_and_the_other_path(eng, tables, join, keyset):
    a, b = tables
    keys = KEYSETS[keyset]
    q = query(join, ON["intersects"], keys)
    out = run(eng, q, a, b, join_aggregates=True)
    want = reference(a, b, _pairs(a, b), keys, join == "LEFT")
    check(out, want, keys)
    if join == "LEFT" and keyset == "interval":      # an unmatched row: COUNT(*) = 1, COUNT(col) = 0, SUM NULL
        assert any(row[0][0] == 1 and row[1][0] == 0 and row[3][0] is None for row in want.values())
    if join == "LEFT" and keyset == "chrom":         # a key with unmatched rows only: one padded row each
        assert [x[0] for x in want[("chrQ",)][:4]] == [3, 0, 0, None]
    assert out.schema.types[len(keys):] == [pa.int64(), pa.int64(), pa.int64(), pa.float64(), pa.float64(), pa.float64(),
                                            pa.int32(), pa.int64()]
    if join == "INNER":     # the query runs without the flag too: the same table
        old = run(eng, q, a, b)
        check(old, want, keys)
        assert_same_tables(out, old, keys)


def test_left_without_a_count_item_equals_the_padded_path(eng, tables):
    a, b = tables
    aggs = [x for x in AGGS if x[0] != "COUNT"]
    for keys in KEYSETS.values():
        q = query("LEFT", ON["intersects"], keys, aggs)
        out = run(eng, q, a, b, join_aggregates=True)
        want = reference(a, b, _pairs(a, b), keys, True, aggs)
        check(out, want, keys, aggs)
        old = run(eng, q, a, b, outer_joins=True)
        check(old, want, keys, aggs)
        assert_same_tables(out, old, keys)
        assert_same_tables(out, run(eng, q, a, b, outer_joins=True, join_aggregates=True), keys)


@pytest.mark.parametrize("predicate", ["contains", "within", "distance"])
def test_the_other_pair_predicates(eng, tables, predicate):
    a, b = tables
    keys = KEYSETS["interval"]
    pairs = _pairs(a, b, predicate)
    assert pairs
    for join in ("INNER", "LEFT"):
        q = query(join, ON[predicate], keys)
        out = run(eng, q, a, b, join_aggregates=True)
        want = reference(a, b, pairs, keys, join == "LEFT")
        check(out, want, keys)
        if join == "INNER":
            old = run(eng, q, a, b)
            check(old, want, keys)
            assert_same_tables(out, old, keys)


def test_a_strand_residual_in_on(eng, tables):
    a, b = tables
    keys = KEYSETS["name"]
    pairs = _pairs(a, b, strand=True)
    for join in ("INNER", "LEFT"):
        q = query(join, ON["intersects"] + " AND a.strand = b.strand", keys)
        out = run(eng, q, a, b, join_aggregates=True)
        want = reference(a, b, pairs, keys, join == "LEFT")
        check(out, want, keys)
        if join == "INNER":
            old = run(eng, q, a, b)
            check(old, want, keys)
            assert_same_tables(out, old, keys)
    # the lone COUNT beside a residual: declines without the flag, counts with it (unmatched rows: 0)
    lone = [("COUNT", "name", "n_name")]
    q = query("LEFT", ON["intersects"] + " AND a.strand = b.strand", KEYSETS["interval"], lone)
    out = run(eng, q, a, b, join_aggregates=True)
    check(out, reference(a, b, pairs, KEYSETS["interval"], True, lone), KEYSETS["interval"], lone)


def test_having_order_by_and_limit_ride_on_the_grouped_result(eng, tables):
    a, b = tables
    aggs = [("SUM", "weight", "w"), ("COUNT", "*", "c")]
    tail = " HAVING COUNT(b.score) > 2 AND MAX(b.weight) > 0 ORDER BY w DESC, a.name LIMIT 4 OFFSET 1"
    q = query("INNER", ON["intersects"], KEYSETS["name"], aggs, tail)
    out = run(eng, q, a, b, join_aggregates=True)
    old = run(eng, q, a, b)
    assert out.column_names == ["name", "w", "c"] and out.num_rows == 4
    assert out.to_pydict() == old.to_pydict()
    want = reference(a, b, _pairs(a, b), KEYSETS["name"], False,
                     aggs + [("COUNT", "score", "h0"), ("MAX", "weight", "h1")])
    kept = [(k[0], r[0][0], r[1][0]) for k, r in want.items() if r[2][0] > 2 and r[3][0] is not None and r[3][0] > 0]
    kept.sort(key=lambda x: (-x[1], x[0] is not None, x[0]))
    assert list(zip(*(out.column(c).to_pylist() for c in out.column_names))) == kept[1:5]
    # DISTINCT over the grouped result
    q = f"SELECT DISTINCT a.chrom, COUNT(*) AS c FROM a JOIN b ON {ON['intersects']} GROUP BY a.chrom"
    assert sorted(run(eng, q, a, b, join_aggregates=True).to_pylist(), key=repr) == sorted(run(eng, q, a, b).to_pylist(), key=repr)


def test_outside_the_shape_execute_answers_as_without_the_flag(eng, tables):
    from giql_amd.transpile import HipDeclined

    a, b = tables
    # MIN of a string column: the plan is marked, its types are not the shape's -- the other path answers
    q = f"SELECT a.chrom, MIN(b.name) AS first, COUNT(*) AS c FROM a JOIN b ON {ON['intersects']} GROUP BY a.chrom"
    assert sorted(run(eng, q, a, b, join_aggregates=True).to_pylist(), key=repr) == sorted(run(eng, q, a, b).to_pylist(), key=repr)
    # ... and where the query declines without the flag, it declines with it, in the same words
    q = f"SELECT a.chrom, MIN(b.name) AS first, COUNT(b.score) AS c FROM a LEFT JOIN b ON {ON['intersects']} GROUP BY a.chrom"
    with pytest.raises(HipDeclined) as without:
        run(eng, q, a, b)
    with pytest.raises(HipDeclined) as with_flag:
        run(eng, q, a, b, join_aggregates=True)
    assert str(with_flag.value) == str(without.value)
    # return_indices: the pairs of the join, as without the flag
    q = query("INNER", ON["intersects"], KEYSETS["chrom"])
    ra, rb = run(eng, q, a, b, join_aggregates=True, return_indices=True)
    assert sorted(zip(ra.tolist(), rb.tolist())) == sorted(_pairs(a, b))


def test_an_integer_sum_that_could_overflow_refuses(eng, tables):
    a, b = tables
    big = pa.array([2**62 if w is not None else None for w in b["weight"]], pa.int64())
    tb = {"a": _arrow(a), "b": _arrow(b).set_column(6, "weight", big)}
    from giql_amd.execute import execute

    q = query("INNER", ON["intersects"], KEYSETS["chrom"], [("SUM", "weight", "w")])
    with pytest.raises(ValueError, match="can overflow the int64 sum"):
        execute(q, tb, eng, giql_tables=T, join_aggregates=True)
    q = query("INNER", ON["intersects"], KEYSETS["chrom"], [("MAX", "weight", "w")])
    assert set(execute(q, tb, eng, giql_tables=T, join_aggregates=True).column("w").to_pylist()) == {2**62}


def test_a_genome_wider_than_the_32_bit_axis(eng):
    """Two chromosomes whose rows lie at both ends of the int32 range: the join falls back to its grouped retry, the
    pairs it returns are aggregated as any others."""
    r = np.random.default_rng(36)
    tabs = []
    for n, names in ((200, ["g1", "g2", "g3"]), (500, ["x", "y"])):
        t = _table(r, n, names, chroms=("chr0", "chr1"))
        start = np.where(r.random(n) < 0.5, r.integers(0, 40_000, n), 2_147_000_000 + r.integers(0, 40_000, n))
        end = start + r.integers(1, 600, n)
        start[:2], end[:2] = [0, 2**31 - 101], [100, 2**31 - 1]
        t["chrom"][:2] = ["chr0", "chr1"]
        t["start"], t["end"] = start.tolist(), end.tolist()
        tabs.append(t)
    a, b = tabs
    for join in ("INNER", "LEFT"):
        for keys in (KEYSETS["interval"], KEYSETS["name"]):
            q = query(join, ON["intersects"], keys)
            out = run(eng, q, a, b, join_aggregates=True)
            check(out, reference(a, b, _pairs(a, b), keys, join == "LEFT"), keys)
    assert_same_tables(run(eng, query("INNER", ON["intersects"], KEYSETS["name"]), a, b, join_aggregates=True),
                       run(eng, query("INNER", ON["intersects"], KEYSETS["name"]), a, b), KEYSETS["name"])


def test_nan_scores_through_the_combine_of_a_key_s_rows(eng, tables):
    """NaN is above every number (DuckDB's order): MAX of a key with a NaN is NaN, MIN skips NaNs unless nothing else
    is there, SUM / AVG propagate -- within a left row on the device and across the rows of a key on the host."""
    a, b = tables
    r = np.random.default_rng(5)
    score = list(b["score"])
    for j in r.choice(len(score), 120, replace=False):
        score[j] = float("nan")
    b = dict(b, score=score)
    a = dict(a, name=["only_nan" if i % 50 == 7 else n for i, n in enumerate(a["name"])])
    pairs = _pairs(a, b)
    only = {i for i, n in enumerate(a["name"]) if n == "only_nan"}
    for i, j in pairs:                     # a key whose every non-NULL score is a NaN
        if i in only and score[j] is not None:
            score[j] = float("nan")
    aggs = [("MIN", "score", "lo_score"), ("MAX", "score", "hi"), ("SUM", "score", "s_score"), ("COUNT", "score", "n_score")]
    for join in ("INNER", "LEFT"):
        for keys in (KEYSETS["name"], KEYSETS["chrom"], KEYSETS["interval"]):
            want = reference(a, b, pairs, keys, join == "LEFT", aggs)
            got = _rows(run(eng, query(join, ON["intersects"], keys, aggs), a, b, join_aggregates=True), keys, aggs)
            assert sorted(got, key=repr) == sorted(want, key=repr)
            for key, row in want.items():
                for (w, _xs), g, (func, _c, _n) in zip(row, got[key], aggs):
                    if w is None or w == w:
                        assert func == "SUM" or g == w, (key, func, g, w)      # (SUM: checked by the other tests)
                    else:
                        assert g is not None and g != g, (key, func, g)
    by_name = reference(a, b, pairs, KEYSETS["name"], False, aggs)
    lo, hi = by_name[("only_nan",)][0][0], by_name[("only_nan",)][1][0]
    assert lo != lo and hi != hi                                              # MIN of NaNs alone: NaN
    assert any(r[0][0] == r[0][0] and r[1][0] != r[1][0] for r in by_name.values())   # MIN a number, MAX NaN


def test_a_pinned_table_s_index_serves_the_pairs(eng, tables):
    """Without a residual an INTERSECTS join reads a pinned table's index, with the flag as without it."""
    from giql_amd.execute import execute, pin

    a, b = tables
    keys = KEYSETS["name"]
    with pin(_arrow(b), index=True) as pb:
        for join in ("INNER", "LEFT"):
            out = execute(query(join, ON["intersects"], keys), {"a": _arrow(a), "b": pb}, eng, giql_tables=T,
                          join_aggregates=True)
            check(out, reference(a, b, _pairs(a, b), keys, join == "LEFT"), keys)


# ---------------------------------------------------------------- the sqlite-minted rows
@pytest.mark.parametrize("case", GOLDEN["cases"], ids=lambda c: c["name"])
def test_the_golden_rows(eng, case):
    cols = GOLDEN["columns"]
    a, b = ({c: [r[i] for r in GOLDEN[t]] for i, c in enumerate(cols)} for t in ("a", "b"))
    aggs = [(f, c, f"x{i}") for i, (f, c) in enumerate(GOLDEN["aggregates"])]
    on = ON["intersects"] + (" AND a.strand = b.strand" if case["strand"] else "")
    out = run(eng, query(case["join"], on, case["keys"], aggs), a, b, join_aggregates=True)
    names = case["keys"] + [n for _f, _c, n in aggs]
    got = [list(r) for r in zip(*(out.column(c).to_pylist() for c in names))]
    key = lambda r: [(x is not None, x) for x in r[:len(case["keys"])]]
    assert sorted(got, key=key) == sorted(case["rows"], key=key)    # (quarters: every sum and mean is exact)
