"""SEMI / ANTI / COUNT over CONTAINS, WITHIN and DISTANCE <= N, without a GPU: the ``row_predicates`` keyword's
lowering matrix, what still declines, the C ABI's new symbols, the reduction helper, and the conditions the golden
fixtures must meet for the GPU tests built on them to mean something."""

import os
import re

import numpy as np
import pytest

import _contain_ref as CR
import _distance_ref as DR
import _rows_ref as RR
from giql_amd import _lib
from giql_amd.plan import JoinPlan
from giql_amd.shape import HipDeclined
from giql_amd.transpile import build_plan, transpile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = "DISTANCE(a.interval, b.interval)"
D_FLIPPED = "DISTANCE(b.interval, a.interval)"
COUNT_Q = ("SELECT a.chrom, a.start, a.end, COUNT(b.start) AS n FROM genes a LEFT JOIN variants b ON {on} "
           "GROUP BY a.chrom, a.start, a.end")
ROW_Q = "SELECT a.name FROM genes a {kind} JOIN variants b ON {on}"

# (ON clause, the plan's predicate, its max_distance)
PREDICATES = [
    ("a.interval CONTAINS b.interval", "contains", None),
    ("a.interval WITHIN b.interval", "within", None),
    ("b.interval CONTAINS a.interval", "within", None),         # operands the other way round flip, as for INNER
    ("b.interval WITHIN a.interval", "contains", None),
    (D + " <= 5", "within_distance", 5),
    (D + " < 5", "within_distance", 4),
    (D_FLIPPED + " <= 0", "within_distance", 0),
    (D + " < 0", "within_distance", -1),
]


def _queries(on):
    return [("SEMI", ROW_Q.format(kind="SEMI", on=on)), ("ANTI", ROW_Q.format(kind="ANTI", on=on)),
            ("COUNT", COUNT_Q.format(on=on))]


# ------------------------------------------------------------------ the lowering matrix
@pytest.mark.parametrize("on, predicate, max_distance", PREDICATES, ids=[p[0] for p in PREDICATES])
def test_keyword_lowers_every_kind_over_every_predicate(on, predicate, max_distance):
    for kind, q in _queries(on):
        plan = build_plan(q, None, row_predicates=True)
        assert (plan.kind, plan.predicate, plan.max_distance, plan.row_predicates) == (kind, predicate, max_distance, True)
        assert plan.left.table == "genes" and plan.right.table == "variants" and not plan.residuals
        text = transpile(q, None, dialect="hip", row_predicates=True)
        assert text == plan.to_string() and JoinPlan.from_string(text) == plan
        assert JoinPlan.from_dict(plan.to_dict()) == plan


def test_default_still_declines_with_the_pinned_messages():
    for on, label in (("a.interval CONTAINS b.interval", "CONTAINS"), ("a.interval WITHIN b.interval", "WITHIN"),
                      (D + " <= 5", "DISTANCE")):
        for kind, q in _queries(on):
            reason = f"count_overlaps over {label}" if kind == "COUNT" else f"{kind} join over {label}"
            for kw in ({}, {"outer_joins": True}, {"row_predicates": False}):
                with pytest.raises(HipDeclined, match=reason):
                    build_plan(q, None, **kw)
            with pytest.raises(HipDeclined, match=reason):
                transpile(q, None, dialect="hip")


def test_keyword_changes_nothing_else():
    for q in ("SELECT a.name FROM genes a SEMI JOIN variants b ON a.interval INTERSECTS b.interval",
              COUNT_Q.format(on="a.interval INTERSECTS b.interval"),
              "SELECT a.name, b.name AS bn FROM genes a JOIN variants b ON a.interval CONTAINS b.interval",
              "SELECT a.name, b.name AS bn FROM genes a JOIN variants b ON " + D + " <= 3"):
        plan = build_plan(q, None)
        assert build_plan(q, None, row_predicates=True) == plan and not plan.row_predicates
        assert "row_predicates" in plan.to_dict()


def test_a_plan_string_written_before_the_field_loads_without_it():
    plan = build_plan("SELECT a.name FROM genes a SEMI JOIN variants b ON a.interval INTERSECTS b.interval", None)
    d = plan.to_dict()
    assert d.pop("row_predicates") is False
    assert JoinPlan.from_dict(d) == plan
    # the mark is what lets a per-row plan carry a pair predicate, and it belongs to nothing else
    row = build_plan(ROW_Q.format(kind="SEMI", on="a.interval CONTAINS b.interval"), None, row_predicates=True).to_dict()
    with pytest.raises(ValueError, match="needs an INNER plan"):
        JoinPlan.from_dict({**row, "row_predicates": False})
    with pytest.raises(ValueError, match="row_predicates marks"):
        JoinPlan.from_dict({**row, "kind": "INNER"})
    with pytest.raises(ValueError, match="row_predicates marks"):
        JoinPlan.from_dict({**row, "predicate": "intersects"})


@pytest.mark.parametrize("query, reason", [
    (COUNT_Q.format(on="a.interval CONTAINS b.interval AND a.score > 1"), "count_overlaps with predicates beside"),
    (COUNT_Q.format(on=D + " <= 5") + " HAVING COUNT(b.start) > 1", "HAVING / ORDER BY / LIMIT over count_overlaps"),
    ("SELECT a.name, " + D + " AS d FROM genes a SEMI JOIN variants b ON a.interval CONTAINS b.interval",
     "SEMI join with a DISTANCE in the SELECT list"),
    ("SELECT a.chrom, a.start, a.end, COUNT(b.start) AS n, " + D + " AS d FROM genes a LEFT JOIN variants b ON "
     + D + " <= 5 GROUP BY a.chrom, a.start, a.end", "count_overlaps / outer join with a DISTANCE in the SELECT list"),
    (ROW_Q.format(kind="SEMI", on="DISTANCE(a.interval, b.interval, signed := true) <= 5"),
     "signed / stranded DISTANCE in a join condition"),
    (ROW_Q.format(kind="ANTI", on="DISTANCE(a.interval, b.interval, stranded := true) <= 5"),
     "signed / stranded DISTANCE in a join condition"),
    ("SELECT a.name FROM genes a SEMI JOIN genes b ON a.interval CONTAINS b.interval", "self-join"),
    ("SELECT a.name FROM genes a SEMI JOIN variants b WHERE a.interval CONTAINS b.interval",
     "SEMI/ANTI join with its INTERSECTS outside ON"),
    ("SELECT a.name FROM genes a SEMI JOIN variants b ON a.interval CONTAINS b.interval AND " + D + " <= 5",
     "more than one spatial predicate in a join"),
    ("SELECT a.name FROM genes a LEFT JOIN variants b ON a.interval WITHIN b.interval WHERE b.chrom IS NULL",
     "LEFT outer join"),
])
def test_what_still_declines_with_the_keyword(query, reason):
    with pytest.raises(HipDeclined, match=re.escape(reason)):
        build_plan(query, None, row_predicates=True)


def test_semi_anti_keep_their_residuals_and_refuse_right_columns():
    q = ROW_Q.format(kind="SEMI", on=D + " <= 5 AND a.score > b.score AND b.score > 1 AND a.score < 9") + " WHERE a.score > 2"
    plan = build_plan(q, None, row_predicates=True)
    assert plan.kind == "SEMI" and plan.predicate == "within_distance" and plan.max_distance == 5
    assert sorted(r.clause for r in plan.residuals) == ["on", "on", "on", "where"]
    assert JoinPlan.from_string(plan.to_string()) == plan
    with pytest.raises(ValueError, match="right side of a SEMI/ANTI join"):
        build_plan("SELECT b.name FROM genes a SEMI JOIN variants b ON a.interval CONTAINS b.interval", None,
                   row_predicates=True)


@pytest.mark.parametrize("on, predicate, max_distance", PREDICATES[:2] + PREDICATES[4:6], ids=lambda x: str(x))
def test_the_v_shortcut_needs_both_switches(on, predicate, max_distance):
    q = f"SELECT a.name FROM genes a LEFT JOIN variants b ON {on} WHERE b.chrom IS NULL AND a.score > 3"
    plan = build_plan(q, None, outer_joins=True, row_predicates=True)
    assert (plan.kind, plan.predicate, plan.max_distance, plan.row_predicates) == ("ANTI", predicate, max_distance, True)
    assert [r.clause for r in plan.residuals] == ["where"]
    left = build_plan(q, None, outer_joins=True)             # without the keyword: the LEFT plan, as before
    assert left.kind == "LEFT" and left.predicate == predicate and not left.row_predicates
    with pytest.raises(HipDeclined, match="LEFT outer join"):
        build_plan(q, None, row_predicates=True)
    # something else reads the right table: an outer join after all
    q2 = f"SELECT a.name, b.name AS bn FROM genes a LEFT JOIN variants b ON {on} WHERE b.chrom IS NULL"
    assert build_plan(q2, None, outer_joins=True, row_predicates=True).kind == "LEFT"


# ------------------------------------------------------------------ the C ABI
def test_header_lib_and_library_agree_on_the_new_symbols():
    text = open(os.path.join(ROOT, "include", "giql_hip.h")).read()
    for name, value in (("GIQL_ROWPRED_CONTAINS", 1), ("GIQL_ROWPRED_WITHIN", 2), ("GIQL_ROWPRED_DISTANCE", 3)):
        assert int(re.search(rf"#define {name}\s+(\d+)", text).group(1)) == value
    assert (_lib.ROWPRED_CONTAINS, _lib.ROWPRED_WITHIN, _lib.ROWPRED_DISTANCE) == (1, 2, 3)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib.load()
    for sym in ("giql_hip_semi_anti_pred_dev", "giql_hip_count_pred_dev"):
        assert re.search(rf"\bint {sym}\s*\(", code), sym
        assert sym in _lib.SYMBOLS and hasattr(L, sym)
    assert int(re.search(r"#define GIQL_HIP_ABI_VERSION (\d+)", text).group(1)) == 4 == L.giql_hip_abi_version()
    assert len(L.giql_hip_semi_anti_pred_dev.argtypes) == 10 and len(L.giql_hip_count_pred_dev.argtypes) == 8


def test_engine_methods_check_their_predicate_before_any_device_call():
    from giql_amd.engine import HipEngine

    eng = HipEngine.__new__(HipEngine)          # no context: the argument checks come first
    assert eng._row_predicate("contains", None) == (1, 0, 0) and eng._row_predicate("within", 7) == (2, 0, 0)
    assert eng._row_predicate("within_distance", 1 << 70) == (3, (1 << 63) - 1, 2)
    assert eng._row_predicate("within_distance", -1) == (3, -1, 2)
    for bad in (("intersects", None), ("within_distance", None), ("within_distance", -2)):
        with pytest.raises(ValueError):
            eng._row_predicate(*bad)


# ------------------------------------------------------------------ the reduction helper
def test_reduce_pairs():
    semi, anti, counts = RR.reduce_pairs([[3, 0], [1, 5], [3, 2], [3, 2]], 5)
    assert semi.tolist() == [1, 3] and anti.tolist() == [0, 2, 4] and counts.tolist() == [0, 1, 0, 3, 0]
    semi, anti, counts = RR.reduce_pairs([], 2)
    assert semi.tolist() == [] and anti.tolist() == [0, 1] and counts.tolist() == [0, 0]
    semi, anti, counts = RR.reduce_pairs(np.zeros((0, 2)), 0)
    assert semi.size == anti.size == counts.size == 0
    assert RR.transpose([[1, 2], [3, 4]]).tolist() == [[2, 1], [4, 3]]


def test_window_counts_agrees_with_the_distance_reference():
    r = np.random.default_rng(5)
    n = 300
    ac, bc = r.integers(0, 3, n), r.integers(0, 3, n)
    as_, bs = r.integers(0, 4000, n), r.integers(0, 4000, n)
    ae, be = as_ + r.integers(0, 40, n), bs + r.integers(0, 40, n)      # zero-length rows among them
    for N in (0, 1, 25, 1 << 40):
        want = RR.reduce_pairs(DR.window_pairs(ac, as_, ae, bc, bs, be, N), n)[2]
        assert np.array_equal(RR.window_counts(ac, as_, ae, bc, bs, be, N, chunk=1000), want) and want.max() >= 1


# ------------------------------------------------------------------ the fixtures are not degenerate
def test_the_containment_fixture_exercises_all_three_reductions():
    cases = CR.golden_cases()
    assert len(cases) >= 100
    both = {"contains": 0, "within": 0}
    multi = {"contains": 0, "within": 0}
    for case in cases:
        for word in both:
            semi, anti, counts = RR.reduce_pairs(case[word], len(case["a"]))
            both[word] += bool(semi.size and anti.size)
            multi[word] += bool(counts.size and counts.max() >= 2)
            assert case[word] == CR.case_brute_force(case, word)
    assert both["contains"] >= 75 and both["within"] >= 60, both
    assert multi["contains"] >= 75 and multi["within"] >= 60, multi


def test_the_distance_fixture_exercises_both_sets_at_every_small_n():
    """All 6 random cases have a non-empty SEMI and a non-empty ANTI set at N in {0, 1, 2}, and a non-empty SEMI set at
    N = 50.  At N = 50 the ANTI set is non-empty in 5 of the 6: every one of random-04's 9 left rows has a neighbour
    within 50 bp (its ANTI result there is the empty one, which the GPU test still compares)."""
    g = DR.golden()
    assert len(g["random"]) == 6 and set(g["within_n"]) >= {0, 1, 2, 50}
    full_at_50 = []
    for case in g["random"]:
        for n in (0, 1, 2, 50):
            semi, anti, counts = RR.reduce_pairs(case["within"][str(n)], len(case["a"]))
            assert semi.size and counts.max() >= 1, (case["id"], n)
            if n < 50:
                assert anti.size, (case["id"], n)
            elif not anti.size:
                full_at_50.append(case["id"])
    assert full_at_50 == ["random-04"]
