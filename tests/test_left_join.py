"""LEFT [OUTER] JOIN in the mirror front end: opt-in lowering, the -v shortcut, the unchanged decline matrix.
No GPU needed."""

import pytest

import _left_ref as R

from giql_amd.plan import JoinPlan
from giql_amd.shape import JoinShape, SelItem, ColRef, TableRef, lower_join_shape
from giql_amd.table import build_tables
from giql_amd.transpile import HipDeclined, build_plan, transpile

T = ["peaks", "genes"]
ON = "a.interval INTERSECTS b.interval"

# bedtools -loj with explicit columns (docs/recipes/bedtools-migration.rst of the reference names the recipe)
Q_LOJ = f"SELECT a.chrom, a.start, a.end, a.name, b.start AS b_start, b.name AS b_name FROM peaks a LEFT JOIN genes b ON {ON}"
# bedtools -v
Q_V = f"SELECT a.chrom, a.start, a.end FROM peaks a LEFT JOIN genes b ON {ON} WHERE b.chrom IS NULL"
Q_NAME_NULL = f"SELECT a.chrom, a.start FROM peaks a LEFT JOIN genes b ON {ON} WHERE b.name IS NULL"
Q_RESIDUALS = (f"SELECT a.name, b.name AS b_name FROM peaks a LEFT OUTER JOIN genes b ON {ON} AND a.score > 3 "
               f"AND b.score < 9 AND a.score < b.score WHERE a.start > 10 AND (b.score > 5 OR a.score = 1)")
Q_AGG = (f"SELECT a.chrom, COUNT(*) AS n, SUM(b.score) AS s, MIN(b.score) AS lo, MAX(b.score) AS hi, AVG(b.score) AS m "
         f"FROM peaks a LEFT JOIN genes b ON {ON} GROUP BY a.chrom")
Q_ORDER = (f"SELECT DISTINCT a.name, b.score FROM peaks a LEFT JOIN genes b ON {ON} "
           f"ORDER BY b.score DESC NULLS LAST, a.name LIMIT 7")
Q_CONTAINS = "SELECT a.name, b.name AS b_name FROM peaks a LEFT JOIN genes b ON a.interval CONTAINS b.interval"
Q_WITHIN = "SELECT a.name, b.name AS b_name FROM peaks a LEFT JOIN genes b ON b.interval CONTAINS a.interval"
Q_DISTANCE = "SELECT a.name, b.name AS b_name FROM peaks a LEFT JOIN genes b ON DISTANCE(a.interval, b.interval) <= 40"

LEFT_QUERIES = [Q_LOJ, Q_V, Q_NAME_NULL, Q_RESIDUALS, Q_AGG, Q_ORDER, Q_CONTAINS, Q_WITHIN, Q_DISTANCE]


@pytest.mark.parametrize("query", LEFT_QUERIES)
def test_without_the_switch_every_left_join_declines_as_before(query):
    with pytest.raises(HipDeclined, match="LEFT outer join"):
        build_plan(query, T)
    with pytest.raises(HipDeclined, match="LEFT outer join"):
        build_plan(query, T, outer_joins=False)
    with pytest.raises(HipDeclined, match="LEFT outer join"):
        transpile(query, T, dialect="hip")


def test_loj_recipe_lowers_to_a_left_plan_and_round_trips():
    plan = build_plan(Q_LOJ, T, outer_joins=True)
    assert plan.kind == "LEFT" and plan.predicate == "intersects" and not plan.residuals
    assert [(p.side, p.column, p.name) for p in plan.projection] == [
        ("l", "chrom", "chrom"), ("l", "start", "start"), ("l", "end", "end"), ("l", "name", "name"),
        ("r", "start", "b_start"), ("r", "name", "b_name")]
    text = transpile(Q_LOJ, T, dialect="hip", outer_joins=True)
    assert text == plan.to_string() and '"kind":"LEFT"' in text
    assert JoinPlan.from_string(text) == plan
    assert build_plan(Q_LOJ.replace("LEFT JOIN", "LEFT OUTER JOIN"), T, outer_joins=True) == plan


@pytest.mark.parametrize("key", ["chrom", "start", "end"])
def test_v_recipe_lowers_to_the_anti_plan(key):
    plan = build_plan(Q_V.replace("b.chrom IS NULL", f"b.{key} IS NULL"), T, outer_joins=True)
    assert plan.kind == "ANTI" and not plan.residuals
    assert plan == build_plan(f"SELECT a.chrom, a.start, a.end FROM peaks a ANTI JOIN genes b ON {ON}", T)


def test_v_recipe_keeps_on_and_where_residuals_in_their_clauses():
    q = (f"SELECT a.name FROM peaks a LEFT JOIN genes b ON {ON} AND b.score > 2 AND a.score < b.score "
         f"WHERE a.score > 1 AND b.start IS NULL ORDER BY a.name LIMIT 3")
    plan = build_plan(q, T, outer_joins=True)
    assert plan.kind == "ANTI"
    assert [(r.clause, r.lhs.kind, r.op) for r in plan.residuals] == [("on", "r", ">"), ("on", "l", "<"), ("where", "l", ">")]
    assert plan.order_by == (("name", False, True),) and plan.limit == 3


@pytest.mark.parametrize("query", [
    Q_NAME_NULL,                                                                    # not a key column: it has NULLs of its own
    f"SELECT a.chrom, b.name FROM peaks a LEFT JOIN genes b ON {ON} WHERE b.chrom IS NULL",      # projects a right column
    f"SELECT a.chrom FROM peaks a LEFT JOIN genes b ON {ON} WHERE b.chrom IS NULL AND b.score IS NULL",
    f"SELECT a.chrom FROM peaks a LEFT JOIN genes b ON {ON} WHERE b.chrom IS NULL OR a.score > 3",
    f"SELECT a.chrom FROM peaks a LEFT JOIN genes b ON {ON} WHERE b.chrom IS NULL ORDER BY b.score",
    f"SELECT a.chrom, COUNT(*) AS n FROM peaks a LEFT JOIN genes b ON {ON} WHERE b.chrom IS NULL GROUP BY a.chrom "
    f"HAVING MAX(b.score) IS NULL",
    "SELECT a.chrom FROM peaks a LEFT JOIN genes b ON a.interval CONTAINS b.interval WHERE b.chrom IS NULL",
])
def test_anything_else_that_reads_the_right_table_stays_left(query):
    assert build_plan(query, T, outer_joins=True).kind == "LEFT"


def test_on_conjuncts_are_on_and_where_conjuncts_are_where():
    plan = build_plan(Q_RESIDUALS, T, outer_joins=True)
    assert plan.kind == "LEFT"
    got = [(r.clause, r.lhs.kind, r.lhs.value, r.op, r.rhs.kind, r.group) for r in plan.residuals]
    assert got == [("on", "l", "score", ">", "int", 0), ("on", "r", "score", "<", "int", 0),
                   ("on", "l", "score", "<", "r", 0), ("where", "l", "start", ">", "int", 0),
                   ("where", "r", "score", ">", "int", 1), ("where", "l", "score", "=", "int", 1)]
    assert JoinPlan.from_string(plan.to_string()) == plan


@pytest.mark.parametrize("query,predicate,max_distance", [
    (Q_CONTAINS, "contains", None), (Q_WITHIN, "within", None), (Q_DISTANCE, "within_distance", 40),
    ("SELECT a.name FROM peaks a LEFT JOIN genes b ON a.interval WITHIN b.interval", "within", None)])
def test_every_pair_predicate_lowers(query, predicate, max_distance):
    plan = build_plan(query, T, outer_joins=True)
    assert (plan.kind, plan.predicate, plan.max_distance) == ("LEFT", predicate, max_distance)
    assert JoinPlan.from_string(plan.to_string()) == plan


def test_distance_join_absorbs_the_chrom_equality_in_on_but_not_in_where():
    q = ("SELECT a.name FROM peaks a LEFT JOIN genes b ON a.chrom = b.chrom AND DISTANCE(a.interval, b.interval) <= 5 "
         "WHERE a.chrom = b.chrom")
    plan = build_plan(q, T, outer_joins=True)
    assert [(r.clause, r.op) for r in plan.residuals] == [("where", "=")]     # the WHERE one drops the padded rows


def test_outer_clauses_ride_on_a_left_plan():
    plan = build_plan(Q_AGG, T, outer_joins=True)
    assert plan.kind == "LEFT" and plan.group_by == ("chrom",)
    assert [(a.func, a.side, a.column) for a in plan.aggregates] == [
        ("COUNT", "*", "*"), ("SUM", "r", "score"), ("MIN", "r", "score"), ("MAX", "r", "score"), ("AVG", "r", "score")]
    plan = build_plan(Q_ORDER, T, outer_joins=True)
    assert plan.kind == "LEFT" and plan.distinct and plan.limit == 7
    assert plan.order_by == (("score", True, False), ("name", False, True))


@pytest.mark.parametrize("query", [
    f"SELECT a.start FROM peaks a RIGHT JOIN genes b ON {ON}",
    f"SELECT a.start FROM peaks a FULL OUTER JOIN genes b ON {ON}",
    f"SELECT a.start FROM peaks a FULL JOIN genes b ON {ON}",
    # the count_overlaps look-alikes: a COUNT(b.col) item keeps the count_overlaps gate, switch or no switch
    f"SELECT COUNT(b.chrom) AS n FROM peaks a LEFT JOIN genes b ON {ON}",
    f"SELECT a.chrom, COUNT(b.chrom) AS n FROM peaks a LEFT JOIN genes b ON {ON} GROUP BY a.chrom ORDER BY a.chrom",
    f"SELECT a.chrom, COUNT(b.chrom) AS n FROM peaks a LEFT JOIN genes b ON {ON} GROUP BY a.chrom, a.start",
    f"SELECT a.chrom, COUNT(b.chrom) AS n FROM peaks a LEFT JOIN genes b ON {ON} WHERE a.score > 1 GROUP BY a.chrom",
    f"SELECT a.chrom, COUNT(b.chrom) FROM peaks a LEFT JOIN genes b ON {ON} GROUP BY a.chrom",
    f"SELECT a.chrom, b.start, COUNT(b.chrom) AS n FROM peaks a LEFT JOIN genes b ON {ON} GROUP BY a.chrom",
    f"SELECT a.chrom, COUNT(b.chrom) AS n FROM peaks a LEFT JOIN genes b ON {ON} GROUP BY a.chrom HAVING COUNT(b.chrom) > 1",
    f"SELECT a.chrom, COUNT(b.chrom) AS n, SUM(b.score) AS s FROM peaks a LEFT JOIN genes b ON {ON} GROUP BY a.chrom",
    # star projections, a self-join, a DISTANCE select item
    f"SELECT * FROM peaks a LEFT JOIN genes b ON {ON}",
    f"SELECT a.*, b.name FROM peaks a LEFT JOIN genes b ON {ON}",
    f"SELECT a.start FROM peaks a LEFT JOIN peaks b ON {ON}",
    f"SELECT a.name, DISTANCE(a.interval, b.interval) AS d FROM peaks a LEFT JOIN genes b ON {ON}",
    "SELECT a.name, DISTANCE(a.interval, b.interval) AS d FROM peaks a LEFT JOIN genes b ON DISTANCE(a.interval, b.interval) <= 9",
    # the predicate in WHERE filters the padded rows away again
    f"SELECT a.start FROM peaks a LEFT JOIN genes b USING (chrom) WHERE {ON}",
])
def test_these_decline_with_the_switch_too(query):
    with pytest.raises(HipDeclined):
        build_plan(query, T, outer_joins=True)
    with pytest.raises(HipDeclined):
        build_plan(query, T)


def test_count_overlaps_is_chosen_before_the_switch_is_read():
    q = f"SELECT a.chrom, a.start, COUNT(b.chrom) AS n FROM peaks a LEFT JOIN genes b ON {ON} GROUP BY a.chrom, a.start"
    assert build_plan(q, T, outer_joins=True) == build_plan(q, T)
    assert build_plan(q, T).kind == "COUNT"


def test_the_switch_changes_nothing_else():
    for q in (f"SELECT a.start FROM peaks a JOIN genes b ON {ON}", f"SELECT a.start FROM peaks a SEMI JOIN genes b ON {ON}",
              f"SELECT a.start FROM peaks a LEFT ANTI JOIN genes b ON {ON} WHERE a.score > 2"):
        assert build_plan(q, T, outer_joins=True) == build_plan(q, T)


def test_join_shape_carries_the_switch():
    def shape(**kw):
        a, b = ColRef("a", False, "interval"), ColRef("b", False, "interval")
        return JoinShape(items=[SelItem(ColRef("a", False, "start"))], from_ref=TableRef("peaks", "a"),
                         join_ref=TableRef("genes", "b"), kind="LEFT", on_seen=True, on_terms=[("intersects", a, b)], **kw)

    assert shape().outer_joins is False
    with pytest.raises(HipDeclined, match="LEFT outer join"):
        lower_join_shape(shape(), build_tables(T))
    assert lower_join_shape(shape(outer_joins=True), build_tables(T)).kind == "LEFT"


def test_left_plans_refuse_what_only_inner_plans_take():
    plan = build_plan(Q_CONTAINS, T, outer_joins=True)
    d = plan.to_dict()
    d["kind"] = "ANTI"
    with pytest.raises(ValueError, match="needs an INNER plan"):
        JoinPlan.from_dict(d)


def test_the_execute_cases_cover_what_they_are_named_for():
    """The fixture's own shape, from SQLite alone: matched and padded rows, padded rows that a WHERE keeps and
    drops, and a left-only ON conjunct whose failing rows are still output."""
    pytest.importorskip("pyarrow")
    tables = R.make_tables()

    def rows(case):
        return R.sqlite_rows(tables, R.giql_and_sql(R.CASES[case])[1])

    loj = rows("loj")
    padded = [r for r in loj if r[4] is None]
    assert padded and len(padded) < len(loj) and len(loj) > tables["peaks"].num_rows
    assert any(r[3] is None and r[4] is not None for r in loj)               # a matched row whose b.name is NULL
    assert all(r[4] is not None for r in rows("where_right")) and all(r[4] is not None for r in rows("where_not"))
    assert any(r[4] is None for r in rows("where_name_is_null")) and any(r[4] is not None for r in rows("where_name_is_null"))
    assert any(r[4] is None for r in rows("where_or_mixed"))
    low = [r for r in rows("on_left_only") if r[2] is None or r[2] <= 5]
    assert low and all(r[4] is None for r in low)                              # failing left rows: output, padded
    assert len(rows("v")) == len(padded)
    assert all(r[2] is None for r in rows("group_all_padded"))
