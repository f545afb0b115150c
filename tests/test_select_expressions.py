"""Computed SELECT-list columns (``select_expressions``), the host side: parsing and lowering of the -wo / -wao
recipes, the plan's serialised form, every decline, the reference ``_expr_ref`` against rows minted by sqlite3
(``tests/golden/make_select_expressions.py``) and against hand-written truth tables, and the coverage of the generator
the GPU test draws from.  No GPU, no HIP library."""
import json
import math
import os

import numpy as np
import pytest

import _expr_ref as R
import _sel_ref
from giql_amd.plan import JoinPlan, Operand, Projection
from giql_amd.shape import HipDeclined
from giql_amd.transpile import build_plan, transpile

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "select_expressions.json")))
ON = "a.interval INTERSECTS b.interval"
OVERLAP = ["fn", "-", [["fn", "least", [["l", "end"], ["r", "end"]]], ["fn", "greatest", [["l", "start"], ["r", "start"]]]]]

WO = ("SELECT a.*, b.*, (LEAST(a.end, b.end) - GREATEST(a.start, b.start)) AS overlap_bp "
      "FROM features_a a, features_b b WHERE a.interval INTERSECTS b.interval")
WAO = ("SELECT a.*, b.*, CASE WHEN b.chrom IS NULL THEN 0 "
       "ELSE LEAST(a.end, b.end) - GREATEST(a.start, b.start) END AS overlap_bp "
       "FROM features_a a LEFT JOIN features_b b ON a.interval INTERSECTS b.interval")
KW = {"outer_joins": True, "select_expressions": True}


# ------------------------------------------------------------------------------------- parsing and lowering
def test_the_wo_recipe_lowers_to_an_inner_plan_with_one_expression():
    plan = build_plan(WO, select_expressions=True)
    assert plan.kind == "INNER" and plan.predicate == "intersects" and not plan.residuals
    assert plan.projection == (Projection("l", "*", "*"), Projection("r", "*", "*"), Projection("expr", "0", "overlap_bp"))
    assert plan.expressions == (Operand("expr", OVERLAP),)


def test_the_wao_recipe_lowers_to_a_left_plan_whose_case_is_an_if_node():
    plan = build_plan(WAO, **KW)
    assert plan.kind == "LEFT" and plan.predicate == "intersects"
    assert plan.projection[-1] == Projection("expr", "0", "overlap_bp")
    assert plan.expressions == (Operand("expr", ["fn", "if", [["fn", "isnull", [["r", "chrom"]]], ["int", 0], OVERLAP]]),)


def test_a_case_with_several_whens_and_no_else_nests_and_ends_in_null():
    q = ("SELECT a.name, CASE WHEN a.score > 5 THEN 1 WHEN b.strand = '+' AND NOT a.score < b.score THEN a.score * 2.5 "
         f"WHEN a.end IS NULL THEN -a.end END w, (a.end) AS e FROM features_a a JOIN features_b b ON {ON}")
    plan = build_plan(q, select_expressions=True)
    assert [p.name for p in plan.projection] == ["name", "w", "e"]
    assert plan.projection[2] == Projection("l", "end", "e")          # a parenthesised plain column stays a column
    third = ["fn", "if", [["fn", "isnull", [["l", "end"]]], ["fn", "neg", [["l", "end"]]], ["fn", "null", []]]]
    second = ["fn", "if", [["fn", "and", [["fn", "=", [["r", "strand"], ["str", "+"]]], ["fn", ">=", [["l", "score"], ["r", "score"]]]]],
                           ["fn", "*", [["l", "score"], ["float", 2.5]]], third]]
    assert plan.expressions[0].value == ["fn", "if", [["fn", ">", [["l", "score"], ["int", 5]]], ["int", 1], second]]


PAIR_JOINS = [(f"JOIN features_b b ON {ON}", "INNER", "intersects"),
              ("JOIN features_b b ON a.interval CONTAINS b.interval", "INNER", "contains"),
              ("JOIN features_b b ON b.interval CONTAINS a.interval", "INNER", "within"),
              ("JOIN features_b b ON DISTANCE(a.interval, b.interval) <= 10", "INNER", "within_distance"),
              (f", features_b b WHERE {ON}", "INNER", "intersects"),
              (f"LEFT JOIN features_b b ON {ON} AND a.score > 1 WHERE b.score IS NULL OR b.score < 3", "LEFT", "intersects"),
              ("LEFT OUTER JOIN features_b b ON a.interval CONTAINS b.interval", "LEFT", "contains"),
              ("LEFT JOIN features_b b ON a.interval WITHIN b.interval", "LEFT", "within"),
              ("LEFT JOIN features_b b ON DISTANCE(a.interval, b.interval) < 11", "LEFT", "within_distance")]


@pytest.mark.parametrize("join,kind,predicate", PAIR_JOINS)
def test_inner_and_left_plans_over_all_four_predicates(join, kind, predicate):
    plan = build_plan(f"SELECT a.name, a.score * b.score AS p, b.end - a.start AS d FROM features_a a {join}", **KW)
    assert (plan.kind, plan.predicate) == (kind, predicate)
    assert [e.value[1] for e in plan.expressions] == ["*", "-"]
    assert [(p.side, p.column) for p in plan.projection] == [("l", "name"), ("expr", "0"), ("expr", "1")]
    assert JoinPlan.from_string(plan.to_string()) == plan


def test_the_plan_string_round_trips_and_older_strings_load():
    for q, kw in ((WO, {"select_expressions": True}), (WAO, KW)):
        plan = build_plan(q, **kw)
        text = transpile(q, dialect="hip", **kw)
        assert text == plan.to_string() and JoinPlan.from_string(text) == plan
        assert JoinPlan.from_dict(json.loads(json.dumps(plan.to_dict()))) == plan
    old = build_plan(f"SELECT a.name FROM features_a a JOIN features_b b ON {ON}")
    d = old.to_dict()
    assert d.pop("expressions") == []
    assert JoinPlan.from_dict(d) == old and JoinPlan.from_dict(d).expressions == ()
    with pytest.raises(ValueError, match="names expression"):
        JoinPlan("INNER", old.left, old.right, (Projection("expr", "0", "x"),))
    with pytest.raises(ValueError, match="INNER or LEFT"):
        JoinPlan("SEMI", old.left, old.right, (), expressions=(Operand("expr", OVERLAP),))


def test_order_by_alias_limit_and_distinct_ride_on_the_output_names():
    plan = build_plan(f"SELECT DISTINCT a.name, a.end - a.start AS w FROM features_a a JOIN features_b b ON {ON} "
                      "ORDER BY w DESC, a.name LIMIT 5 OFFSET 2", select_expressions=True)
    assert plan.distinct and plan.order_by == (("w", True, False), ("name", False, True)) and (plan.limit, plan.offset) == (5, 2)


# ------------------------------------------------------------------------------------- declines
BASE = f"FROM features_a a JOIN features_b b ON {ON}"
DECLINES = [
    (f"SELECT a.name, CASE a.score WHEN 1 THEN 2 END AS w {BASE}", "simple CASE (CASE <value> WHEN ...) in the SELECT list"),
    (f"SELECT a.name, a.score > 5 AS w {BASE}", "comparison or boolean as the value of a SELECT item"),
    (f"SELECT a.name, (a.score > 5) AS w {BASE}", "comparison or boolean as the value of a SELECT item"),
    (f"SELECT a.name, NOT a.score AS w {BASE}", "comparison or boolean as the value of a SELECT item"),
    (f"SELECT a.name, a.score IS NULL AS w {BASE}", "comparison or boolean as the value of a SELECT item"),
    (f"SELECT a.name, CASE WHEN a.score > 5 THEN a.score < 2 END AS w {BASE}", "comparison or boolean as the value of a SELECT item"),
    (f"SELECT a.name, CASE WHEN a.score > 5 THEN 'hi' ELSE 'lo' END AS w {BASE}", "string-valued expression in the SELECT list"),
    (f"SELECT a.name, CASE WHEN a.interval INTERSECTS b.interval THEN 1 END AS w {BASE}", "spatial predicate in a CASE condition"),
    (f"SELECT a.name, DISTANCE(a.interval, b.interval) + 1 AS w {BASE}", "DISTANCE inside an expression of the SELECT list"),
    (f"SELECT a.name, CASE WHEN DISTANCE(a.interval, b.interval) <= 5 THEN 1 END AS w {BASE}",
     "DISTANCE inside an expression of the SELECT list"),
    (f"SELECT a.name, a.end - a.start AS w, COUNT(*) AS c {BASE} GROUP BY a.name",
     "expression in the SELECT list beside GROUP BY / HAVING / aggregates"),
    (f"SELECT a.name, a.end - a.start AS w {BASE} GROUP BY a.name", "expression in the SELECT list beside GROUP BY / HAVING / aggregates"),
    (f"SELECT a.name, COUNT(b.name) AS c, a.end - a.start AS w FROM features_a a LEFT JOIN features_b b ON {ON} GROUP BY a.name",
     "expression in the SELECT list beside GROUP BY / HAVING / aggregates"),
    (f"SELECT a.name, SUM(a.end - a.start) AS w {BASE} GROUP BY a.name", "aggregate over an expression"),
    (f"SELECT a.name, a.end - a.start AS w FROM features_a a SEMI JOIN features_b b ON {ON}", "SEMI join with an expression in the SELECT list"),
    (f"SELECT a.name, a.end - a.start AS w FROM features_a a ANTI JOIN features_b b ON {ON}", "ANTI join with an expression in the SELECT list"),
    (f"SELECT a.name, a.end - a.start AS w FROM features_a a LEFT JOIN features_b b ON {ON} WHERE b.chrom IS NULL",
     "ANTI join with an expression in the SELECT list"),
    ("SELECT a.name, a.end - a.start AS w FROM features_a a CROSS JOIN LATERAL NEAREST(features_b, reference := a.interval, k := 1) b",
     "expression in the SELECT list of a NEAREST join"),
    ("SELECT a.end - a.start AS w, CLUSTER(interval) AS c FROM features_a a", "expression in the SELECT list of CLUSTER / MERGE"),
    ("SELECT a.end - a.start AS w, MERGE(interval) FROM features_a a", "expression in the SELECT list of CLUSTER / MERGE"),
    ("SELECT a.end - a.start AS w FROM DISJOIN(features_a) a", "expression in the SELECT list of DISJOIN"),
    ("SELECT a.end - a.start AS w FROM features_a a WHERE a.interval INTERSECTS 'chr1:1-100'",
     "expression in the SELECT list of a literal-range filter"),
    (f"SELECT a.name, 1 + 2 AS w {BASE}", "constant expression in the SELECT list"),
    (f"SELECT a.name, 7 AS w {BASE}", "constant expression in the SELECT list"),
    (f"SELECT a.name, a.end - a.start {BASE}", "expression without an alias in the SELECT list"),
    (f"SELECT a.name, (a.end - a.start) {BASE}", "expression without an alias in the SELECT list"),
    (f"SELECT a.name, a.end % 2 AS w {BASE}", "operator '%' in an expression of the SELECT list"),
    (f"SELECT a.name, SQRT(a.end) + 1 AS w {BASE}", "function call in an expression of the SELECT list"),
    (f"SELECT a.name, COUNT(b.name) + 1 AS w {BASE}", "function call in an expression of the SELECT list"),
    (f"SELECT DISTINCT a.*, a.end - a.start AS w {BASE}", "star projection"),
    (f"SELECT *, a.end - a.start AS w {BASE}", "star projection"),
]


@pytest.mark.parametrize("query,message", DECLINES, ids=[f"{i}:{m[:40]}" for i, (_q, m) in enumerate(DECLINES)])
def test_what_still_declines_says_why(query, message):
    with pytest.raises(HipDeclined) as exc:
        build_plan(query, **KW)
    assert str(exc.value).startswith(message + ":"), str(exc.value)


def test_user_mistakes_stay_value_errors():
    with pytest.raises(ValueError, match="Unqualified column 'score'"):
        build_plan(f"SELECT a.name, score + 1 AS w {BASE}", **KW)
    with pytest.raises(ValueError, match="Unknown table qualifier 'c'"):
        build_plan(f"SELECT a.name, c.score + 1 AS w {BASE}", **KW)
    with pytest.raises(ValueError, match="expected END"):
        build_plan(f"SELECT a.name, CASE WHEN a.score > 1 THEN 2 AS w {BASE}", **KW)
    with pytest.raises(ValueError, match="expected THEN"):
        build_plan(f"SELECT a.name, CASE WHEN a.score > 1 ELSE 2 END AS w {BASE}", **KW)


# without the keyword nothing changes: the text each query is answered with before the feature existed
TODAY = [
    (WO, HipDeclined, 'expression in the SELECT list'),
    (WAO, ValueError, "Parse error: expected FROM near 'b'"),
    (f'SELECT a.name, (a.end - a.start) AS w {BASE}', HipDeclined, 'expression in the SELECT list'),
    (f'SELECT a.name, a.end - a.start AS w {BASE}', HipDeclined, 'expression in the SELECT list'),
    (f'SELECT a.name, 1 + a.end AS w {BASE}', HipDeclined, 'expression in the SELECT list'),
    (f'SELECT a.name, LEAST(a.end, b.end) AS w {BASE}', HipDeclined, 'function call in the SELECT list'),
    (f'SELECT a.name, CASE WHEN b.chrom IS NULL THEN 0 ELSE 1 END AS w {BASE}', ValueError, "Parse error: expected FROM near 'b'"),
    (f'SELECT a.name, -a.end AS w {BASE}', ValueError, "Parse error: expected an identifier near '-'"),
    (f'SELECT a.end - a.start AS w FROM DISJOIN(features_a) a', HipDeclined, 'expression in the SELECT list'),
    (f'SELECT a.end - a.start AS w, CLUSTER(interval) AS c FROM features_a a', HipDeclined, 'expression in the SELECT list'),
    (f"SELECT a.end - a.start AS w FROM features_a a WHERE a.interval INTERSECTS 'chr1:1-100'", HipDeclined, 'expression in the SELECT list'),
]
# ... and every query of DECLINES, in its order
TODAY_DECLINES = [
    (ValueError, "Parse error: expected FROM near '.'"),
    (HipDeclined, 'expression in the SELECT list'),
    (HipDeclined, 'expression in the SELECT list'),
    (HipDeclined, 'projection starting with NOT'),
    (ValueError, "Parse error: expected FROM near 'IS'"),
    (ValueError, "Parse error: expected FROM near 'a'"),
    (ValueError, "Parse error: expected FROM near 'a'"),
    (ValueError, "Parse error: expected FROM near 'a'"),
    (HipDeclined, 'expression in the SELECT list'),
    (ValueError, "Parse error: expected FROM near 'DISTANCE'"),
    (HipDeclined, 'expression in the SELECT list'),
    (HipDeclined, 'expression in the SELECT list'),
    (HipDeclined, 'expression in the SELECT list'),
    (HipDeclined, 'aggregate over an expression'),
    (HipDeclined, 'expression in the SELECT list'),
    (HipDeclined, 'expression in the SELECT list'),
    (HipDeclined, 'expression in the SELECT list'),
    (HipDeclined, 'expression in the SELECT list'),
    (HipDeclined, 'expression in the SELECT list'),
    (HipDeclined, 'expression in the SELECT list'),
    (HipDeclined, 'expression in the SELECT list'),
    (HipDeclined, 'expression in the SELECT list'),
    (HipDeclined, 'expression in the SELECT list'),
    (HipDeclined, 'expression in the SELECT list'),
    (HipDeclined, 'expression in the SELECT list'),
    (HipDeclined, 'expression in the SELECT list'),
    (ValueError, "Parse error: expected FROM near '%'"),
    (HipDeclined, 'function call in the SELECT list'),
    (HipDeclined, 'expression in the SELECT list'),
    (HipDeclined, 'expression in the SELECT list'),
    (HipDeclined, 'expression in the SELECT list'),
]
TODAY += [(q, k, t) for (q, _m), (k, t) in zip(DECLINES, TODAY_DECLINES)]
assert len(TODAY_DECLINES) == len(DECLINES)


@pytest.mark.parametrize("k", range(len(TODAY)))
def test_without_the_keyword_every_query_is_answered_as_before(k):
    query, kind, text = TODAY[k]
    for kw in ({}, {"outer_joins": True}, {"outer_joins": True, "row_predicates": True}):
        with pytest.raises(ValueError) as exc:
            build_plan(query, **kw)
        assert type(exc.value) is kind, (type(exc.value), str(exc.value))
        assert str(exc.value).split(": this query")[0] == text, str(exc.value)
    with pytest.raises(ValueError) as exc:
        transpile(query, dialect="hip")
    assert type(exc.value) is kind


# ------------------------------------------------------------------------------------- golden rows (sqlite3)
COLS = GOLDEN["columns"]
STRINGS = ("chrom", "name", "strand")


class _Bound:
    """A plan's expressions as ``_expr_ref`` trees over numpy columns (left = side "a"); strings under a comparison
    become ranks in one sorted dictionary shared by both operands (binary collation), as ``execute()`` binds them."""

    def __init__(self, fa, fb):
        self.rows = {"l": fa, "r": fb}

    def _vals(self, side, col):
        return [r[COLS.index(col)] for r in self.rows[side]]

    def _is_str(self, t):
        return t[0] == "str" or (t[0] in ("l", "r") and t[1] in STRINGS)

    def _column(self, side, col, code=None):
        vals = self._vals(side, col)
        valid = np.array([v is not None for v in vals], np.uint8)
        if code is not None:
            data = np.array([code.get(v, 0) for v in vals], np.int32)
        elif col in STRINGS:
            data = np.zeros(len(vals), np.uint8)                        # only its validity is read
        elif col == "weight":
            data = np.array([0.0 if v is None else v for v in vals], np.float64)
        else:
            data = np.array([0 if v is None else v for v in vals], np.int64)
        return ("a" if side == "l" else "b", data, valid)

    def tree(self, t):
        if t[0] != "fn":
            return ("lit", t[1]) if t[0] in ("int", "float") else self._column(t[0], t[1])
        op, kids = t[1], t[2]
        if op in _sel_ref.CMP and any(self._is_str(k) for k in kids):
            words = set()
            for k in kids:
                words |= {k[1]} if k[0] == "str" else {v for v in self._vals(k[0], k[1]) if v is not None}
            code = {w: j for j, w in enumerate(sorted(words))}
            return (op, *[("lit", code[k[1]]) if k[0] == "str" else self._column(k[0], k[1], code) for k in kids])
        return (op, *[self.tree(k) for k in kids])


def _joined(case):
    """The row ids the join leaves, by the predicate spelt out: the pairs, then (LEFT) every unmatched left row."""
    fa, fb = case["features_a"], case["features_b"]

    def distance(p, g):
        return 0 if p[1] < g[2] and p[2] > g[1] else (g[1] - p[2] + 1 if p[2] <= g[1] else p[1] - g[2] + 1)

    test = {"intersects": lambda p, g: p[1] < g[2] and p[2] > g[1], "contains": lambda p, g: p[1] <= g[1] and p[2] >= g[2],
            "within": lambda p, g: p[1] >= g[1] and p[2] <= g[2], "distance": lambda p, g: distance(p, g) <= 40}[case["join"]]
    pairs = [(i, j) for i, p in enumerate(fa) for j, g in enumerate(fb) if p[0] == g[0] and test(p, g)]
    if case["left"]:
        pairs += [(i, -1) for i in sorted(set(range(len(fa))) - {i for i, _ in pairs})]
    return pairs


def _key(r):
    return tuple((x is None, x) for x in r)


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=[c["id"] for c in GOLDEN["cases"]])
def test_the_reference_gives_the_golden_rows_through_the_plans_expressions(case):
    plan = build_plan(case["query"], **KW)
    assert plan.kind == ("LEFT" if case["left"] else "INNER")
    assert [p.name for p in plan.projection if p.side == "expr"] == case["aliases"]
    fa, fb = case["features_a"], case["features_b"]
    pairs = _joined(case)
    ia, ib = (np.array([p[k] for p in pairs], np.int64) for k in (0, 1))
    bound = _Bound(fa, fb)
    cols = []
    for e in plan.expressions:
        vals, valid = R.evaluate(bound.tree(e.value), ia, ib)
        cols.append([None if not ok else (float(v) if vals.dtype == np.float64 else int(v)) for v, ok in zip(vals, valid)])
    got = [[fa[i][3], fa[i][1], fb[j][3] if j >= 0 else None, fb[j][2] if j >= 0 else None, *[c[k] for c in cols]]
           for k, (i, j) in enumerate(pairs)]
    want = case["rows"]
    assert len(got) == len(want)
    for g, w in zip(sorted(got, key=_key), want):
        assert g[:4] == w[:4]
        for x, y in zip(g[4:], w[4:]):
            assert type(x) is type(y) and x == y, (case["id"], g, w)       # floats bit for bit: one rounded operation each


def test_the_golden_cases_cover_what_they_should():
    ids = {c["id"].rsplit("-", 1)[0] for c in GOLDEN["cases"]}
    assert {"wo", "wao", "wo-contains", "wo-within", "wo-distance", "case-on-a-string", "float-product", "fraction"} <= ids
    rows = [r for c in GOLDEN["cases"] for r in c["rows"]]
    assert any(r[2] is None for r in rows) and any(r[4] is None for r in rows) and any(isinstance(r[4], float) for r in rows)
    wao = [r for c in GOLDEN["cases"] if c["id"].startswith("wao-") for r in c["rows"]]
    assert all(r[4] == 0 for r in wao if r[2] is None) and any(r[2] is None for r in wao)
    dist = [r[4] for c in GOLDEN["cases"] if c["join"] == "distance" for r in c["rows"]]
    assert min(dist) < 0 and 0 in dist and max(dist) > 0                    # apart, touching, overlapping


# ------------------------------------------------------------------------------------- if / null truth tables
def _one(tree, ia=(0,), ib=(0,)):
    vals, valid = R.evaluate(tree, np.array(ia), np.array(ib))
    return [None if not ok else v.item() for v, ok in zip(vals, valid)], vals.dtype


def test_if_and_null_truth_tables():
    T, F, N = (">", ("lit", 1), ("lit", 0)), ("<", ("lit", 1), ("lit", 0)), (">", ("null",), ("lit", 0))
    i1, i2, f1, f2, nul = ("lit", 4), ("lit", -7), ("lit", 0.5), ("lit", -2.25), ("null",)
    for cond, takes_then in ((T, True), (F, False), (N, False)):
        for then, other in ((i1, i2), (i1, f2), (f1, i2), (f1, f2), (i1, nul), (nul, i2), (f1, nul), (nul, f2), (nul, nul)):
            got, dtype = _one(("if", cond, then, other))
            chosen = then if takes_then else other
            is_float = any(isinstance(b[1], float) for b in (then, other) if b[0] == "lit")
            assert dtype == (np.float64 if is_float else np.int64)              # `then OR else`, whichever is taken
            want = None if chosen == nul else (float(chosen[1]) if is_float else chosen[1])
            assert got == [want] and type(got[0]) is type(want), (cond, then, other, got)
    # a number as the condition: TRUE unless zero, a NaN included; NULL is not TRUE
    for v, takes_then in ((3, True), (0, False), (-0.0, False), (math.nan, True), (0.25, True)):
        assert _one(("if", ("lit", v), ("lit", 1), ("lit", 2)))[0] == [1 if takes_then else 2]
    # `null` is an integer NULL and propagates; IS NULL sees it; LEAST skips it
    assert _one(("+", nul, ("lit", 1))) == ([None], np.int64)
    assert _one(("isnull", nul))[0] == [1] and _one(("least", nul, ("lit", 3)))[0] == [3]
    assert _one(("/", ("lit", 1), ("lit", 0))) == ([None], np.float64)
    # booleans as values are 0 / 1 / NULL integers
    assert _one(T)[0] == [1] and _one(F)[0] == [0] and _one(N) == ([None], np.int64)
    assert _one(("and", N, F))[0] == [0] and _one(("or", N, T))[0] == [1] and _one(("not", N))[0] == [None]


def test_a_negative_id_is_the_null_row_of_its_side():
    a = ("a", np.array([10, 20], np.int64))
    b = ("b", np.array([1.5, 2.5]), np.array([1, 0], np.uint8))
    ia, ib = [0, -1, 1, -1, 1], [0, 1, -1, -1, 1]
    assert _one(a, ia, ib)[0] == [10, None, 20, None, 20]
    assert _one(b, ia, ib)[0] == [1.5, None, None, None, None]
    assert _one(("if", ("isnull", b), ("lit", 0), ("-", a, ("lit", 1))), ia, ib)[0] == [9, 0, 0, 0, 0]
    assert _one(("+", a, b), ia, ib) == ([11.5, None, None, None, None], np.float64)
    assert _one(("least", a, b), ia, ib)[0] == [1.5, None, 20.0, None, 20.0]      # LEAST skips the NULL side
    assert _one(("isnull", a), ia, ib)[0] == [0, 1, 0, 1, 0]
    with pytest.raises(R.Int64Overflow):
        _one(("*", ("a", np.array([2**62], np.int64)), ("lit", 4)))


def test_the_static_type_rule():
    i, f = ("a", np.zeros(1, np.int32)), ("b", np.zeros(1, np.float32))
    floaty = [f, ("lit", 1.0), ("/", i, i), ("+", i, f), ("neg", f), ("abs", ("*", f, i)), ("least", i, f), ("greatest", f, i),
              ("if", ("<", i, f), i, f), ("if", ("<", i, f), f, ("null",)), ("-", ("if", i, ("/", i, i), i), i)]
    inty = [i, ("lit", 1), ("null",), ("+", i, i), ("<", f, f), ("isnull", f), ("notnull", f), ("and", f, f), ("or", f, i),
            ("not", f), ("if", f, i, i), ("if", ("/", i, i), i, ("null",)), ("least", i, ("=", f, f)), ("abs", ("neg", i))]
    assert all(R.can_float(t) for t in floaty) and not any(R.can_float(t) for t in inty)


def test_node_and_live_value_counts_of_if_and_null():
    x = ("lit", 1)
    assert R.count_nodes(("if", x, x, x)) == 4 and R.live_values(("if", x, x, x)) == 3
    assert R.count_nodes(("null",)) == 1 and R.live_values(("if", ("<", x, x), ("null",), ("+", x, x))) == 4
    assert R.live_values(("if", ("if", x, x, x), x, x)) == 3 and R.count_nodes(("+", ("if", x, x, ("null",)), x)) == 6
    # the gate's estimate (shape.expression_cost) agrees on the plan's form
    from giql_amd.shape import expression_cost
    plan = build_plan(WAO, **KW)
    assert expression_cost(plan.expressions[0]) == (11, 5)


# ------------------------------------------------------------------------------------- the generator
@pytest.fixture(scope="module")
def draws():
    return [(seed, n, *R.draw(seed, n)) for seed, n in R.GPU_CASES]


def test_the_generator_reaches_every_case_over_the_gpu_seeds(draws):
    kinds, dtypes, depths, first_depths = set(), set(), set(), set()
    for seed, n, d, ia, ib, expected in draws:
        assert len(d.trees) == 8
        assert all(R.live_values(t) <= 12 and R.count_nodes(t) <= 256 for t in d.trees)
        for t, (vals, valid) in zip(d.trees, expected):
            kinds |= R.node_kinds(t)
            dtypes.add(vals.dtype.name)
            depths.add(R.live_values(t))
        first_depths.add(R.live_values(d.trees[0]))
        # over the population with the NULL rows of either side: NULL and non-NULL values both occur
        pop = d.expected(np.array(d.pa + [-1, 0, -1]), np.array(d.pb + [0, -1, -1]))
        assert any((ok == 0).any() for _v, ok in pop) and any((ok == 1).any() for _v, ok in pop), seed
        if n >= 63:
            assert any((ok == 0).any() for _v, ok in expected) and any((ok == 1).any() for _v, ok in expected), seed
            both = (ia < 0) & (ib < 0)
            assert (ia < 0).any() and (ib < 0).any() and both.any() and ((ia >= 0) & (ib >= 0)).any(), seed
    assert kinds == set(_sel_ref.KINDS) | {"if", "null"}
    assert dtypes == {"int64", "float64"}
    assert {1, 12} <= depths and {1, 12} <= first_depths
    assert any(R.count_nodes(t) == 256 for _s, _n, d, *_ in draws for t in d.trees)


@pytest.mark.parametrize("seed,n,n_trees", [(s, n, 8) for s, n in R.GPU_CASES] + [(22, 2049, k) for k in (1, 2, 8, 9)]
                         + [(25, 2049, 8), (24, 2049, 8), (23, 2049, 8)])
def test_every_seed_the_gpu_test_uses_draws_within_the_attempts(seed, n, n_trees):
    d, ia, ib, expected = R.draw(seed, n, n_trees=n_trees)          # (raises past MAX_ATTEMPTS)
    assert d.attempt < R.MAX_ATTEMPTS == 8 and len(expected) == n_trees and all(len(v) == n for v, _ok in expected)


def test_the_generator_is_a_function_of_its_seed():
    (d1, ia1, ib1, e1), (d2, ia2, ib2, e2) = R.draw(9, 2049), R.draw(9, 2049)
    assert np.array_equal(ia1, ia2) and np.array_equal(ib1, ib2)
    assert all(np.array_equal(R.bits(x[0].astype(np.float64)), R.bits(y[0].astype(np.float64))) and np.array_equal(x[1], y[1])
               for x, y in zip(e1, e2))


def test_flattening_matches_the_counts():
    """``HipEngine._flatten_expr`` lays ``if`` / ``null`` out as the reference counts them (no device needed)."""
    from giql_amd import _lib
    from giql_amd.engine import HipEngine, expr_can_float

    eng = HipEngine.__new__(HipEngine)
    x = ("lit", 1)
    for tree in (("if", ("<", x, ("lit", 2.0)), ("null",), ("+", x, x)), ("+", ("if", x, x, ("null",)), x), ("null",)):
        nodes = []
        eng._flatten_expr(tree, nodes, [])
        assert len(nodes) == R.count_nodes(tree)
        assert expr_can_float(tree) == R.can_float(tree)
    nodes = []
    eng._flatten_expr(("if", x, ("lit", 2), ("null",)), nodes, [])
    assert [nd.side for nd in nodes] == [_lib.SIDE_LIT, _lib.SIDE_LIT, _lib.X_NULL, _lib.X_IF]
    with pytest.raises(ValueError):
        eng._flatten_expr(("if", x, x), [], [])
