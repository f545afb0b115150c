"""DISTANCE on the hip dialect without a GPU: the golden fixture (tests/golden/distance.json, minted by
tests/golden/make_distance.py) against the numpy restatement, the widened-overlap identity the kernels rest on, the
plan of every accepted shape from both front ends, the plan's serialisation, every decline with its reason, the
user errors, and the ABI."""

import ctypes
import json
import os
import re

import numpy as np
import pytest

import _ast_doubles as A
import _distance_ref as R
from giql_amd import _lib, plugin
from giql_amd.plan import PLAN_PREFIX, JoinPlan, Projection
from giql_amd.shape import HipDeclined
from giql_amd.table import Table, build_tables
from giql_amd.transpile import build_plan, transpile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = ["features_a", "features_b"]
RECIPE = ("SELECT a.name, b.name AS b_name, DISTANCE(a.interval, b.interval) AS dist "
          "FROM features_a a CROSS JOIN features_b b "
          "WHERE a.chrom = b.chrom AND DISTANCE(a.interval, b.interval) <= 10000")


# ------------------------------------------------------------------ the fixture and the restatement
def test_fixture_meets_its_conditions():
    g = R.golden()
    assert g["within_n"] == [0, 1, 2, 50, 1 << 40]
    assert len(g["known"]) >= 20 and all(re.fullmatch(r"tests/test_distance_udf\.py:\d+", c["source"]) for c in g["known"])
    assert {c["variant"] for c in g["known"]} == set(R.VARIANTS)
    cases = g["random"]
    assert {tuple(c["enc_a"]) for c in cases} == set(R.OFFSETS) and len({tuple(c["enc_b"]) for c in cases}) >= 3
    for c in cases:
        assert len(c["a"]) <= 64 and len(c["b"]) <= 64
        assert len({r[0] for r in c["a"] + c["b"]}) == 3
        assert {r[3] for r in c["a"] + c["b"]} == {"+", "-", ".", "?", None}
        assert any(r[1] + R.OFFSETS[tuple(c["enc_a"])][0] == r[2] + R.OFFSETS[tuple(c["enc_a"])][1] for r in c["a"])
        assert 0 < len(c["within"]["0"]) < len(c["within"]["1"]) <= len(c["within"]["50"]) <= len(c["pairs"])
        assert c["within"][str(1 << 40)] == c["pairs"]
    assert any({r[0] for r in c["a"]} != {r[0] for r in c["b"]} for c in cases)      # a chromosome on one side only
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "distance.json")) < 100_000


def _case_values(case, variant):
    a, b, _n = R.case_arrays(case)
    (ac, as_, ae), (bc, bs, be) = R.canonical(a), R.canonical(b)
    p = np.array(case["pairs"], np.int64).reshape(-1, 2)
    stranded, signed = R.VARIANTS[variant]
    d, valid = R.distance(ac[p[:, 0]], as_[p[:, 0]], ae[p[:, 0]], bc[p[:, 1]], bs[p[:, 1]], be[p[:, 1]], signed=signed,
                          stranded=stranded, strand_a=a[4][p[:, 0]], strand_b=b[4][p[:, 1]])
    return [int(x) if ok else None for x, ok in zip(d, valid)]


def test_numpy_restatement_reproduces_the_fixture():
    g = R.golden()
    for c in g["random"]:
        for variant in R.VARIANTS:
            assert _case_values(c, variant) == c["values"][variant], (c["id"], variant)
        a, b, _n = R.case_arrays(c)
        for n in g["within_n"]:
            assert R.window_pairs(*R.canonical(a), *R.canonical(b), n).tolist() == c["within"][str(n)], (c["id"], n)
    for k in g["known"]:
        stranded, signed = R.VARIANTS[k["variant"]]
        (ca, sa, ea, ta), (cb, sb, eb, tb) = k["a"], k["b"]
        d, valid = R.distance([0], [sa], [ea], [0 if ca == cb else 1], [sb], [eb], signed=signed, stranded=stranded,
                              strand_a=[R.STRAND_CODE[ta]], strand_b=[R.STRAND_CODE[tb]])
        assert (int(d[0]) if valid[0] else None) == k["expected"], k["source"]


def test_widened_overlap_is_the_predicate_on_well_formed_rows_only():
    """DISTANCE(a, b) <= N  <=>  a.start - N < b.end AND a.end + N > b.start: every quadruple of 0..6 with
    start <= end and N in 0..7 (6272 cases, no mismatch); with an inverted row on either side it fails (756)."""
    v = np.arange(7)
    as_, ae, bs, be, n = (x.ravel() for x in np.meshgrid(v, v, v, v, np.arange(8), indexing="ij"))
    d, _valid = R.distance(0 * as_, as_, ae, 0 * as_, bs, be)
    literal = (as_ - n < be) & (ae + n > bs)
    well = (as_ <= ae) & (bs <= be)
    assert int(well.sum()) == 6272 and not ((d <= n) != literal)[well].any()
    assert int(((d <= n) != literal)[~well].sum()) == 756
    # the clamp: one position beyond the chromosome's range keeps the predicate; a clamp at 0 does not
    a, b, big = (3, 5), (0, 0), 10
    assert R.distance([0], [a[0]], [a[1]], [0], [b[0]], [b[1]])[0][0] == 4
    cmin, cmax = 0, 5
    assert max(a[0] - big, cmin - 1) < b[1] and min(a[1] + big, cmax + 1) > b[0]
    assert not (max(a[0] - big, 0) < b[1])


# ------------------------------------------------------------------ the text front end
def test_the_documented_recipe_lowers_to_a_within_distance_plan():
    text = transpile(RECIPE, TABLES, dialect="hip")       # (declined with "function call in ..." before)
    plan = JoinPlan.from_string(text)
    assert plan.kind == "INNER" and plan.predicate == "within_distance" and plan.max_distance == 10000
    assert (plan.left.table, plan.right.table) == ("features_a", "features_b")
    assert not plan.residuals                              # a.chrom = b.chrom is absorbed
    assert plan.projection == (Projection("l", "name", "name"), Projection("r", "name", "b_name"),
                               Projection("pair_distance", "lr", "dist"))


@pytest.mark.parametrize("frm", ["features_a a CROSS JOIN features_b b WHERE", "features_a a JOIN features_b b ON",
                                 "features_a a, features_b b WHERE", "features_a a INNER JOIN features_b b ON"])
def test_accepted_join_forms(frm):
    plan = build_plan(f"SELECT a.name, b.name AS bn FROM {frm} DISTANCE(a.interval, b.interval) <= 7", TABLES)
    assert (plan.kind, plan.predicate, plan.max_distance) == ("INNER", "within_distance", 7)


def test_operand_order_bounds_and_residuals():
    q = "SELECT a.name FROM features_a a JOIN features_b b ON "
    assert build_plan(q + "DISTANCE(b.interval, a.interval) <= 7", TABLES).max_distance == 7    # symmetric: same plan
    assert build_plan(q + "DISTANCE(b.interval, a.interval) <= 7", TABLES) == \
        build_plan(q + "DISTANCE(a.interval, b.interval) <= 7", TABLES)
    assert build_plan(q + "DISTANCE(a.interval, b.interval) < 7", TABLES).max_distance == 6     # < N is <= N - 1
    assert build_plan(q + "7 >= DISTANCE(a.interval, b.interval)", TABLES).max_distance == 7
    assert build_plan(q + "DISTANCE(a.interval, b.interval) <= 0", TABLES).max_distance == 0
    # < 0 / <= -1: an ordinary empty result, not an error
    assert build_plan(q + "DISTANCE(a.interval, b.interval) < 0", TABLES).max_distance == -1
    assert build_plan(q + "DISTANCE(a.interval, b.interval) <= -1", TABLES).max_distance == -1
    assert build_plan(q + f"DISTANCE(a.interval, b.interval) <= {(1 << 63) - 1}", TABLES).max_distance == (1 << 63) - 1
    plan = build_plan(q + "DISTANCE(a.interval, b.interval) <= 50 AND b.chrom = a.chrom AND a.score > 5 "
                          "AND (a.start < b.start OR b.name = 'x') WHERE b.strand = '+' ORDER BY a.name LIMIT 3", TABLES)
    assert plan.predicate == "within_distance" and plan.limit == 3
    assert [(r.clause, r.op, r.group) for r in plan.residuals] == [("on", ">", 0), ("on", "<", 1), ("on", "=", 1),
                                                                    ("where", "=", 0)]
    # beside INTERSECTS the equality stays what it was: a residual
    plan = build_plan("SELECT a.name FROM features_a a JOIN features_b b ON a.interval INTERSECTS b.interval "
                      "AND a.chrom = b.chrom", TABLES)
    assert [(r.lhs.value, r.op, r.rhs.value) for r in plan.residuals] == [("chrom", "=", "chrom")]


def test_projection_shapes():
    q = "SELECT a.name, {} FROM features_a a JOIN features_b b ON a.interval {} b.interval ORDER BY a.name, d"
    for word in ("INTERSECTS", "CONTAINS", "WITHIN"):
        plan = build_plan(q.format("DISTANCE(a.interval, b.interval) AS d", word), TABLES)
        assert plan.predicate == word.lower() and plan.projection[1] == Projection("pair_distance", "lr", "d")
        assert plan.order_by == (("name", False, True), ("d", False, True)) and plan.strand_col is None
    plan = build_plan(q.format("DISTANCE(b.interval, a.interval, stranded := true, signed := true) d", "INTERSECTS"), TABLES)
    assert plan.projection[1] == Projection("pair_distance", "rl+signed+stranded", "d")
    assert plan.strand_col == "strand,strand"
    plan = build_plan(q.format("DISTANCE(a.interval, b.interval, signed := true) AS d", "INTERSECTS"), TABLES)
    assert plan.projection[1].column == "lr+signed"
    plan = build_plan("SELECT DISTINCT DISTANCE(a.interval, b.interval) FROM features_a a, features_b b "
                      "WHERE DISTANCE(a.interval, b.interval) <= 3 LIMIT 5", TABLES)
    assert plan.distinct and plan.limit == 5 and plan.projection == (Projection("pair_distance", "lr", "distance"),)
    tables = [Table("features_a", strand_col="str_a"), Table("features_b", strand_col="str_b")]
    plan = build_plan(q.format("DISTANCE(a.interval, b.interval, stranded := true) AS d", "INTERSECTS"), tables)
    assert plan.strand_col == "str_a,str_b"


# ------------------------------------------------------------------ the AST front end
def _dist(l=("a", "interval"), r=("b", "interval"), **named):
    return A.N("giqldistance", this=A.col(*l), expression=A.col(*r),
               **{k: A.N("boolean", this=v) for k, v in named.items()})


def _run_plugin(root, node, tables=TABLES):
    tbls = build_tables(list(tables))
    cols = {arg: A.resolved(node.args[arg].args["table"].args["this"], None) for arg in ("this", "expression")}
    ctx = A.ExpansionContext(tables=tbls, resolution=A.OperatorResolution(operator="GIQLDistance", columns=cols))
    calls = []
    expander = plugin.make_distance_expander(lambda n, c: calls.append(n) or "CASE", lambda payload: ("COMMAND", payload))
    return expander(node, ctx), ctx, calls


def test_the_plugin_lowers_the_recipe_to_the_same_plan_as_the_mirror():
    pred, item = _dist(), _dist()
    where = A.conj(A.cmp("eq", A.col("a", "chrom"), A.col("b", "chrom")), A.cmp("lte", pred, A.lit(10000)))
    root = A.select([A.col("a", "name"), A.alias(A.col("b", "name"), "b_name"), A.alias(item, "dist")],
                    A.tbl("features_a", "a"), [A.join(A.tbl("features_b", "b"), kind="CROSS")], where=where)
    for node in (pred, item):            # the expander runs once per DISTANCE node: each leaves the node, same payload
        out, ctx, calls = _run_plugin(root, node)
        assert out is node and not calls and len(ctx.finalizers) == 1
        tag, payload = ctx.finalizers[0](root)
        assert tag == "COMMAND" and JoinPlan.from_string(payload) == build_plan(RECIPE, TABLES)


def test_the_plugin_on_join_lt_swapped_operands_and_projection_beside_intersects():
    pred = _dist(("b", "interval"), ("a", "interval"))
    root = A.select([A.col("a", "name")], A.tbl("features_a", "a"),
                    [A.join(A.tbl("features_b", "b"), on=A.conj(A.cmp("lt", pred, A.lit(5)),
                                                                  A.cmp("gt", A.col("a", "score"), A.lit(3))))])
    out, ctx, calls = _run_plugin(root, pred)
    assert out is pred and not calls
    want = build_plan("SELECT a.name FROM features_a a JOIN features_b b ON DISTANCE(b.interval, a.interval) < 5 "
                      "AND a.score > 3", TABLES)
    assert JoinPlan.from_string(ctx.finalizers[0](root)[1]) == want and want.max_distance == 4
    # the value in the SELECT list of an INTERSECTS join: both expanders reach the same plan
    item = _dist(stranded=True, signed=True)
    inter = A.intersects(A.col("a", "interval"), A.col("b", "interval"))
    root = A.select([A.col("a", "name"), A.alias(item, "d")], A.tbl("features_a", "a"),
                    [A.join(A.tbl("features_b", "b"), on=inter)], order=[(A.col("a", "name"), False), (A.col(None, "d"), False)])
    want = build_plan("SELECT a.name, DISTANCE(a.interval, b.interval, stranded := true, signed := true) AS d "
                      "FROM features_a a JOIN features_b b ON a.interval INTERSECTS b.interval ORDER BY a.name, d", TABLES)
    out, ctx, calls = _run_plugin(root, item)
    assert out is item and JoinPlan.from_string(ctx.finalizers[0](root)[1]) == want
    tbls = build_tables(TABLES)
    cols = {arg: A.resolved(inter.args[arg].args["table"].args["this"], None) for arg in ("this", "expression")}
    ctx = A.ExpansionContext(tables=tbls, resolution=A.OperatorResolution(columns=cols))
    out = plugin.make_expander(lambda n, c: "FALLBACK", lambda p: ("COMMAND", p))(inter, ctx)
    assert out is inter and JoinPlan.from_string(ctx.finalizers[0](root)[1]) == want


def test_the_plugin_falls_back_to_the_case_on_a_decline_and_raises_the_reference_error():
    pred = _dist()
    root = A.select([A.col("a", "name")], A.tbl("features_a", "a"),
                    [A.join(A.tbl("features_b", "b"), on=A.cmp("gt", pred, A.lit(5)))])
    out, ctx, calls = _run_plugin(root, pred)
    assert out == "CASE" and calls == [pred] and not ctx.finalizers
    pred = _dist(signed=True)
    root = A.select([A.col("a", "name")], A.tbl("features_a", "a"),
                    [A.join(A.tbl("features_b", "b"), on=A.cmp("lte", pred, A.lit(5)))])
    assert _run_plugin(root, pred)[0] == "CASE"
    agg = A.agg("min", _dist())
    inter = A.intersects(A.col("a", "interval"), A.col("b", "interval"))
    root = A.select([A.col("a", "name"), agg], A.tbl("features_a", "a"), [A.join(A.tbl("features_b", "b"), on=inter)],
                    group=[A.col("a", "name")])
    with pytest.raises(HipDeclined, match="DISTANCE inside an aggregate"):
        plugin.shape_from_ast(root, inter, A.ExpansionContext(tables=build_tables(TABLES)))
    lit = A.N("giqldistance", this=A.col("a", "interval"), expression=A.lit("chr1:1-2"))
    root = A.select([A.col("a", "name")], A.tbl("features_a", "a"),
                    [A.join(A.tbl("features_b", "b"), on=A.cmp("lte", lit, A.lit(5)))])
    with pytest.raises(ValueError, match="Literal range as second argument not yet supported"):
        plugin.shape_from_ast(root, lit, A.ExpansionContext(tables=build_tables(TABLES)))


def _inter():
    return A.intersects(A.col("a", "interval"), A.col("b", "interval"))


def _plugin_shape(on=None, items=None, where=None, **clauses):
    """shape_from_ast + the gate over a hand-built statement around ``on`` (default: an INTERSECTS join)."""
    inter = _inter()
    root = A.select(items or [A.col("a", "name")], A.tbl("features_a", "a"),
                    [A.join(A.tbl("features_b", "b"), on=A.conj(inter, on) if on is not None else inter)],
                    where=where, **clauses)
    return plugin.lower_statement(root, inter, A.ExpansionContext(tables=build_tables(TABLES)))


def _between(x, lo, hi):
    return A.N("between", this=x, low=lo, high=hi)


SCORE = lambda: A.col("a", "score")


@pytest.mark.parametrize("build, reason", [
    # BETWEEN / IN: the tested value, either bound, arithmetic inside a bound, under NOT
    (lambda: dict(on=_between(_dist(), A.lit(1), A.lit(5))), "BETWEEN / IN over a DISTANCE"),
    (lambda: dict(on=_between(SCORE(), A.lit(1), _dist())), "BETWEEN / IN over a DISTANCE"),
    (lambda: dict(on=_between(SCORE(), _dist(), A.lit(5))), "BETWEEN / IN over a DISTANCE"),
    (lambda: dict(on=_between(SCORE(), A.lit(1), A.N("add", this=_dist(), expression=A.lit(1)))),
     "BETWEEN / IN over a DISTANCE"),
    (lambda: dict(on=A.N("not", this=_between(SCORE(), A.lit(1), _dist()))), "BETWEEN / IN over a DISTANCE"),
    (lambda: dict(where=_between(SCORE(), A.lit(1), _dist())), "BETWEEN / IN over a DISTANCE"),
    (lambda: dict(on=A.N("in", this=_dist(), expressions=[A.lit(1), A.lit(5)])), "BETWEEN / IN over a DISTANCE"),
    # comparisons the join does not take, arithmetic, IS NULL, a non-literal bound
    (lambda: dict(on=A.cmp("gte", _dist(), A.lit(5))), "DISTANCE compared with >="),
    (lambda: dict(on=A.cmp("eq", _dist(), A.lit(5))), "DISTANCE compared with ="),
    (lambda: dict(on=A.cmp("neq", _dist(), A.lit(5))), "DISTANCE compared with !="),
    (lambda: dict(on=A.cmp("lte", SCORE(), _dist())), "DISTANCE compared with >="),
    (lambda: dict(on=A.cmp("lte", A.N("add", this=_dist(), expression=A.lit(1)), A.lit(5))),
     "DISTANCE inside an arithmetic expression"),
    (lambda: dict(on=A.N("is", this=_dist(), expression=A.N("null"))), "IS [NOT] NULL over a DISTANCE"),
    (lambda: dict(on=A.cmp("lte", _dist(), SCORE())), "DISTANCE bound that is not an integer literal"),
    (lambda: dict(on=A.cmp("lte", _dist(), A.lit(5))), "more than one spatial predicate in a join"),
    (lambda: dict(on=A.N("or", this=A.cmp("lte", _dist(), A.lit(5)), expression=A.cmp("gt", SCORE(), A.lit(1)))),
     "spatial predicate under OR"),
    # named arguments
    (lambda: dict(on=A.cmp("lte", A.N("giqldistance", this=A.col("a", "interval"), expression=A.col("b", "interval"),
                                      stranded=A.col("a", "flag")), A.lit(5))), "non-literal stranded / signed argument"),
    (lambda: dict(items=[A.alias(A.N("giqldistance", this=A.col("a", "interval"), expression=A.col("b", "interval"),
                                     signed=A.col("a", "flag")), "d")]), "non-literal stranded / signed argument"),
    # GROUP BY / HAVING / aggregates
    (lambda: dict(group=[_dist()]), "DISTANCE in GROUP BY"),
    (lambda: dict(group=[A.col("a", "name")], having=A.cmp("gt", _dist(), A.lit(1))), "DISTANCE in HAVING"),
    (lambda: dict(group=[A.col("a", "name")],
                  having=A.cmp("gt", A.N("add", this=A.agg("count"), expression=_dist()), A.lit(1))), "DISTANCE in HAVING"),
    (lambda: dict(items=[A.col("a", "name"), A.agg("max", _dist())], group=[A.col("a", "name")]),
     "DISTANCE inside an aggregate"),
    (lambda: dict(items=[A.col("a", "name"), A.alias(_dist(), "d")], group=[A.col("a", "name")]),
     "DISTANCE in the SELECT list beside GROUP BY / HAVING / aggregates"),
])
def test_the_plugin_declines_with_a_reason(build, reason):
    with pytest.raises(HipDeclined, match=re.escape(reason)):
        _plugin_shape(**build())


def test_the_plugin_declines_the_non_literal_bound_and_the_join_kinds():
    def window(on, **kw):
        pred = on
        root = A.select(kw.pop("items", [A.col("a", "name")]), A.tbl("features_a", "a"),
                        [A.join(A.tbl("features_b", "b"), on=pred, **kw)])
        return plugin.lower_statement(root, pred, A.ExpansionContext(tables=build_tables(TABLES)))

    with pytest.raises(HipDeclined, match="DISTANCE bound that is not an integer literal"):
        window(A.cmp("lte", _dist(), SCORE()))
    with pytest.raises(HipDeclined, match="DISTANCE bound that is not an integer literal"):
        window(A.cmp("lte", _dist(), A.lit(2.5)))
    with pytest.raises(HipDeclined, match="SEMI join over DISTANCE"):
        window(A.cmp("lte", _dist(), A.lit(5)), kind="SEMI")
    with pytest.raises(HipDeclined, match="ANTI join over DISTANCE"):
        window(A.cmp("lte", _dist(), A.lit(5)), kind="ANTI")
    with pytest.raises(HipDeclined, match="NOT over a spatial predicate"):
        window(A.N("not", this=A.cmp("lte", _dist(), A.lit(5))))
    with pytest.raises(HipDeclined, match="SEMI join with a DISTANCE in the SELECT list"):
        inter = _inter()
        root = A.select([A.col("a", "name"), A.alias(_dist(), "d")], A.tbl("features_a", "a"),
                        [A.join(A.tbl("features_b", "b"), on=inter, kind="SEMI")])
        plugin.lower_statement(root, inter, A.ExpansionContext(tables=build_tables(TABLES)))
    assert window(A.cmp("lte", _dist(), A.lit(5))).max_distance == 5       # (the helper itself lowers what is accepted)


def test_a_distance_term_is_never_bound_as_a_column():
    """The binding stage refuses a DISTANCE term outright: whatever path hands it one, no plan compares against a
    column named after the genomic pseudo-column."""
    from giql_amd.shape import ColRef, bind_expression, resolve_residual
    from giql_amd.plan import PlanSide

    fn = ("distfn", ColRef("a", False, "interval"), ColRef("b", False, "interval"), False, False)
    left, right = PlanSide("features_a", "a"), PlanSide("features_b", "b")
    for lhs, rhs in ((("col", ColRef("a", False, "score")), fn), (fn, ("lit", 5)),
                     (("col", ColRef("a", False, "score")), ("fn", "+", [fn, ("lit", 1)]))):
        with pytest.raises(HipDeclined, match="DISTANCE as an operand of a condition"):
            resolve_residual("on", ("cmp", lhs, "<=", rhs), left, right, "INNER")
    with pytest.raises(HipDeclined, match="DISTANCE as an operand of a condition"):
        bind_expression(fn, lambda o: None)
    for plan in (build_plan(RECIPE, TABLES), build_plan(Q + "a.interval INTERSECTS b.interval AND a.score BETWEEN 1 AND 5", TABLES)):
        assert not any("interval" in (str(r.lhs.value), str(r.rhs.value)) for r in plan.residuals)


# ------------------------------------------------------------------ the plan
def test_plan_round_trips_and_old_strings_load_unchanged():
    plan = build_plan(RECIPE + " AND a.score > 1 ORDER BY a.name, dist LIMIT 9", TABLES)
    assert plan.to_dict()["predicate"] == "within_distance" and plan.to_dict()["max_distance"] == 10000
    assert JoinPlan.from_string(plan.to_string()) == plan and JoinPlan.from_dict(plan.to_dict()) == plan
    stranded = build_plan("SELECT DISTANCE(a.interval, b.interval, stranded := true) AS d FROM features_a a "
                          "JOIN features_b b ON a.interval INTERSECTS b.interval", TABLES)
    assert JoinPlan.from_string(stranded.to_string()) == stranded and stranded.strand_col == "strand,strand"
    # plan strings written before the change: no "predicate" key at all, and a CONTAINS plan as it was written
    old = build_plan("SELECT a.name FROM features_a a JOIN features_b b ON a.interval INTERSECTS b.interval", TABLES)
    d = old.to_dict()
    assert d.pop("predicate") == "intersects" and d["max_distance"] is None
    assert JoinPlan.from_string(PLAN_PREFIX + json.dumps(d, sort_keys=True, separators=(",", ":"))) == old
    contains = build_plan("SELECT a.name FROM features_a a JOIN features_b b ON a.interval CONTAINS b.interval", TABLES)
    assert JoinPlan.from_string(contains.to_string()).predicate == "contains"
    with pytest.raises(ValueError, match="needs an integer max_distance"):
        JoinPlan("INNER", old.left, old.right, predicate="within_distance")
    with pytest.raises(ValueError, match="needs an INNER plan"):
        JoinPlan("SEMI", old.left, old.right, predicate="within_distance", max_distance=3)


# ------------------------------------------------------------------ what declines, what is an error
Q = "SELECT a.name FROM features_a a JOIN features_b b ON "
D = "DISTANCE(a.interval, b.interval)"


@pytest.mark.parametrize("query, reason", [
    (Q + "DISTANCE(a.interval, b.interval, signed := true) <= 5", "signed / stranded DISTANCE in a join condition"),
    (Q + "DISTANCE(a.interval, b.interval, stranded := true) <= 5", "signed / stranded DISTANCE in a join condition"),
    (Q + D + " > 5", "DISTANCE compared with >"),
    (Q + D + " >= 5", "DISTANCE compared with >="),
    (Q + D + " = 5", "DISTANCE compared with ="),
    (Q + D + " != 5", "DISTANCE compared with !="),
    (Q + "5 < " + D, "DISTANCE compared with >"),
    (Q + D + " BETWEEN 1 AND 5", "BETWEEN / IN over a DISTANCE"),
    (Q + D + " IN (1, 5)", "BETWEEN / IN over a DISTANCE"),
    (Q + D + " NOT BETWEEN 1 AND 5", "BETWEEN / IN over a DISTANCE"),
    # a DISTANCE as a BETWEEN bound, beside INTERSECTS and beside the within-distance predicate
    (Q + "a.interval INTERSECTS b.interval AND a.score BETWEEN 1 AND " + D, "BETWEEN / IN over a DISTANCE"),
    (Q + "a.interval INTERSECTS b.interval AND a.score BETWEEN " + D + " AND 5", "BETWEEN / IN over a DISTANCE"),
    (Q + "a.interval INTERSECTS b.interval AND a.score NOT BETWEEN 1 AND " + D, "BETWEEN / IN over a DISTANCE"),
    (Q + "a.interval INTERSECTS b.interval AND a.score BETWEEN 1 AND " + D + " + 1", "BETWEEN / IN over a DISTANCE"),
    (Q + "a.interval INTERSECTS b.interval AND a.score BETWEEN 2 * " + D + " AND 9", "BETWEEN / IN over a DISTANCE"),
    (Q + D + " <= 5 AND a.score BETWEEN 1 AND " + D, "BETWEEN / IN over a DISTANCE"),
    (Q + "a.interval INTERSECTS b.interval AND a.score <= " + D, "DISTANCE compared with >="),
    (Q + "a.interval INTERSECTS b.interval AND a.score + " + D + " <= 5", "DISTANCE inside an arithmetic expression"),
    (Q + "a.interval INTERSECTS b.interval AND " + D + " IS NULL", "IS [NOT] NULL over a DISTANCE"),
    (Q + D + " <= a.score", "DISTANCE bound that is not an integer literal"),
    (Q + D + " <= 2.5", "DISTANCE bound that is not an integer literal"),
    (Q + D + f" <= {1 << 63}", "DISTANCE bound that does not fit int64"),
    (Q + D + " + 1 <= 5", "DISTANCE inside an arithmetic expression"),
    (Q + D + " <= 5 OR a.score > 1", "spatial predicate under OR"),
    (Q + "NOT " + D + " <= 5", "NOT over a spatial predicate"),
    (Q + D + " <= 5 AND a.interval INTERSECTS b.interval", "more than one spatial predicate in a join"),
    (Q + D + " <= 5 AND a.interval CONTAINS b.interval", "more than one spatial predicate in a join"),
    (Q + D + " <= 5 AND " + D + " <= 9", "more than one spatial predicate in a join"),
    ("SELECT a.name, MIN(" + D + ") FROM features_a a JOIN features_b b ON a.interval INTERSECTS b.interval "
     "GROUP BY a.name", "DISTANCE inside an aggregate"),
    ("SELECT a.name, " + D + " AS d FROM features_a a JOIN features_b b ON a.interval INTERSECTS b.interval "
     "GROUP BY a.name", "DISTANCE in the SELECT list beside GROUP BY / HAVING / aggregates"),
    ("SELECT a.name FROM features_a a JOIN features_b b ON a.interval INTERSECTS b.interval GROUP BY " + D,
     "DISTANCE in GROUP BY"),
    ("SELECT a.name FROM features_a a JOIN features_b b ON a.interval INTERSECTS b.interval GROUP BY a.name "
     "HAVING " + D + " > 1", "DISTANCE in HAVING"),
    ("SELECT a.name FROM features_a a SEMI JOIN features_b b ON " + D + " <= 5", "SEMI join over DISTANCE"),
    ("SELECT a.name FROM features_a a ANTI JOIN features_b b ON " + D + " <= 5", "ANTI join over DISTANCE"),
    ("SELECT a.name, " + D + " AS d FROM features_a a SEMI JOIN features_b b ON a.interval INTERSECTS b.interval",
     "SEMI join with a DISTANCE in the SELECT list"),
    ("SELECT a.chrom, a.start, a.end, COUNT(b.start) AS n FROM features_a a LEFT JOIN features_b b ON " + D + " <= 5 "
     "GROUP BY a.chrom, a.start, a.end", "count_overlaps over DISTANCE"),
    ("SELECT a.name, " + D + " AS d FROM features_a a CROSS JOIN LATERAL NEAREST(features_b, reference := a.interval, "
     "k := 1) b", "DISTANCE in the SELECT list of a NEAREST join"),
    ("SELECT a.name FROM features_a a JOIN features_a b ON " + D + " <= 5", "self-join"),
])
def test_declines_with_a_reason(query, reason):
    with pytest.raises(HipDeclined, match=re.escape(reason)):
        transpile(query, TABLES, dialect="hip")


def test_stranded_distance_needs_a_strand_column_on_both_tables():
    tables = [Table("features_a"), Table("features_b", strand_col=None)]
    with pytest.raises(HipDeclined, match="stranded DISTANCE over a table without a strand column"):
        build_plan("SELECT DISTANCE(a.interval, b.interval, stranded := true) AS d FROM features_a a JOIN features_b b "
                   "ON a.interval INTERSECTS b.interval", tables)
    assert build_plan("SELECT DISTANCE(a.interval, b.interval) AS d FROM features_a a JOIN features_b b "
                      "ON a.interval INTERSECTS b.interval", tables).strand_col is None


def test_user_errors_are_value_errors():
    with pytest.raises(ValueError, match="Literal range as second argument not yet supported") as exc:
        build_plan(Q + "DISTANCE(a.interval, 'chr1:1-2') <= 5", TABLES)
    assert not isinstance(exc.value, HipDeclined)
    with pytest.raises(ValueError, match="Literal range as first argument not yet supported"):
        build_plan("SELECT DISTANCE('chr1:1-2', b.interval) FROM features_a a JOIN features_b b "
                   "ON a.interval INTERSECTS b.interval", TABLES)
    with pytest.raises(ValueError, match="DISTANCE operands must be the tables' genomic columns") as exc:
        build_plan(Q + "DISTANCE(a.start, b.interval) <= 5", TABLES)
    assert not isinstance(exc.value, HipDeclined)
    with pytest.raises(ValueError, match="Unknown table qualifier"):
        build_plan("SELECT DISTANCE(a.interval, c.interval) FROM features_a a JOIN features_b b "
                   "ON a.interval INTERSECTS b.interval", TABLES)


# ------------------------------------------------------------------ the ABI
def test_symbols_header_and_version():
    header = open(os.path.join(ROOT, "include", "giql_hip.h")).read()
    L = _lib.load()
    assert L.giql_hip_abi_version() == 4 and re.search(r"#define GIQL_HIP_ABI_VERSION 4\b", header)
    for sym in ("giql_hip_window_plan_dev", "giql_hip_distance_dev"):
        assert re.search(rf"\bint {sym}\s*\(", header), sym
        assert sym in _lib.SYMBOLS and hasattr(L, sym)
        assert getattr(L, sym).argtypes is not None
    assert "_distance.py:67-117" in header and "distance.py:297-331" in header
    kernels = open(os.path.join(ROOT, "giql_amd", "csrc", "distance_kernels.hip.h")).read()
    assert "_distance.py:67-117" in kernels and "docs/recipes/distance.rst:60-73" in kernels


def test_null_arguments_are_refused_before_any_device_work():
    L = _lib.load()
    n = ctypes.c_int64(-1)
    side = _lib.CSide()
    assert L.giql_hip_window_plan_dev(None, ctypes.byref(side), ctypes.byref(side), 1, 5, None,
                                      ctypes.byref(n)) == _lib.GIQL_ERR_INVALID
    with pytest.raises(_lib.GiqlHipError) as exc:
        _lib.check(L.giql_hip_window_plan_dev(None, None, None, 1, 5, None, None))
    assert exc.value.code == _lib.GIQL_ERR_INVALID and "NULL" in str(exc.value)
    assert L.giql_hip_distance_dev(None, ctypes.byref(side), ctypes.byref(side), None, None, 0, None, None, 0, None,
                                   None, None) == _lib.GIQL_ERR_INVALID
    with pytest.raises(_lib.GiqlHipError) as exc:
        _lib.check(L.giql_hip_distance_dev(None, None, None, None, None, 1, None, None, 0, None, None, None))
    assert exc.value.code == _lib.GIQL_ERR_INVALID and "ctx is NULL" in str(exc.value)
