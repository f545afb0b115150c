"""DISJOIN without a GPU: the front ends, the plan, the declines, the ABI, and the brute-force restatement
against the golden fixture (tests/golden/disjoin.json, minted by tests/golden/make_disjoin.py)."""

import os
import re

import numpy as np
import pytest

import _ast_doubles as D
from _disjoin_ref import brute_force, brute_force_arrays, golden_cases, OFFSETS
from giql_amd import _lib
from giql_amd.plan import DISJOIN_COLUMNS, JoinPlan
from giql_amd.plugin import lower_disjoin_statement
from giql_amd.shape import HipDeclined
from giql_amd.table import Table, build_tables
from giql_amd.transpile import build_plan, transpile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_star_over_disjoin_is_a_disjoin_plan():
    plan = JoinPlan.from_string(transpile("SELECT * FROM DISJOIN(features)", ["features"], dialect="hip"))
    assert plan.kind == "DISJOIN" and plan.left.table == "features" and plan.right is None
    assert [(p.side, p.column) for p in plan.projection] == [("star", "*")]


def test_explicit_reference_and_projection_forms():
    tables = [Table("features", coordinate_system="1based", interval_type="closed"), "refs"]
    plan = build_plan("SELECT f.name, f.disjoin_start AS s, disjoin_chrom FROM DISJOIN(features, reference := refs) AS f "
                      "ORDER BY disjoin_end DESC LIMIT 5 OFFSET 2", tables)
    assert plan.kind == "DISJOIN" and plan.right.table == "refs" and plan.left.encoding == ("1based", "closed")
    assert [(p.side, p.column, p.name) for p in plan.projection] == [
        ("l", "name", "name"), ("disjoin", "disjoin_start", "s"), ("disjoin", "disjoin_chrom", "disjoin_chrom"),
        ("disjoin", "disjoin_end", "__giql_o0")]
    assert plan.order_by == (("__giql_o0", True, False),) and (plan.limit, plan.offset) == (5, 2)


def test_docs_recipe_lowers():
    plan = build_plan("SELECT DISTINCT disjoin_chrom, disjoin_start, disjoin_end FROM DISJOIN(features) "
                      "ORDER BY disjoin_start", ["features"])
    assert plan.distinct and [p.column for p in plan.projection] == list(DISJOIN_COLUMNS)
    assert plan.order_by == (("disjoin_start", False, True),)


@pytest.mark.parametrize("query", [
    "SELECT * FROM DISJOIN(features)",
    "SELECT name, disjoin_end FROM DISJOIN(features, reference := refs) ORDER BY name LIMIT 3",
])
def test_plan_round_trips(query):
    plan = build_plan(query, ["features", "refs"])
    assert JoinPlan.from_dict(plan.to_dict()) == plan
    assert JoinPlan.from_string(plan.to_string()) == plan
    assert plan.to_dict()["kind"] == "DISJOIN"


@pytest.mark.parametrize("query, reason", [
    ("SELECT * FROM DISJOIN((SELECT * FROM features))", "DISJOIN over a sub-query"),
    ("WITH bins AS (SELECT 1) SELECT * FROM DISJOIN(features, reference := bins)", "DISJOIN over a CTE"),
    ("SELECT * FROM DISJOIN(features) JOIN refs ON 1 = 1", "table functions as join operands"),
    ("SELECT * FROM refs JOIN DISJOIN(features) ON 1 = 1", "table functions as join operands"),
    ("SELECT * FROM DISJOIN(__giql_dj_tgt)", "reserved prefix '__giql_dj_'"),
    ("SELECT __giql_dj_x FROM DISJOIN(features)", "reserved prefix '__giql_dj_'"),
    ("SELECT * FROM DISJOIN(features) WHERE disjoin_start > 5", "WHERE over the rows of DISJOIN"),
    ("SELECT COUNT(*) FROM DISJOIN(features)", "aggregates over the rows of DISJOIN"),
    ("SELECT name FROM DISJOIN(features) GROUP BY name", "aggregates over the rows of DISJOIN"),
    ("SELECT * FROM DISJOIN(features, k := 3)", "DISJOIN argument 'k'"),
])
def test_declines_with_a_reason(query, reason):
    with pytest.raises(HipDeclined, match=re.escape(reason)):
        transpile(query, ["features", "refs"], dialect="hip")


def _disjoin_node(target, reference=None):
    return D.N("giqldisjoin", this=D.tbl(target), reference=D.tbl(reference) if reference else None)


def test_plugin_lowering_gives_the_same_plan():
    tables = build_tables([Table("features", coordinate_system="1based", interval_type="closed"), "refs"])
    node = _disjoin_node("features", "refs")
    root = D.select([D.col(None, "name"), D.alias(D.col(None, "disjoin_start"), "s")], node, [],
                    order=[(D.col(None, "disjoin_end"), True, False)], limit=4, distinct=False)
    feats = tables.get("features")
    res = D.OperatorResolution("GIQLDisjoin", columns={"this": D.resolved("features", feats),
                                                        "reference": D.resolved("refs", tables.get("refs"))})
    got = lower_disjoin_statement(root, node, D.ExpansionContext(tables, res))
    want = build_plan("SELECT name, disjoin_start AS s FROM DISJOIN(features, reference := refs) "
                      "ORDER BY disjoin_end DESC LIMIT 4", tables)
    assert got == want
    # self mode, star, DISTINCT
    node = _disjoin_node("features")
    root = D.select([D.star()], node, [], distinct=True)
    assert lower_disjoin_statement(root, node, D.ExpansionContext(tables)) == build_plan(
        "SELECT DISTINCT * FROM DISJOIN(features)", tables)


def test_plugin_declines_like_the_parser():
    tables = build_tables(["features", "refs"])
    node = _disjoin_node("features")
    with pytest.raises(HipDeclined, match="table functions as join operands"):
        lower_disjoin_statement(D.select([D.star()], node, [D.join(D.tbl("refs"))]), node, D.ExpansionContext(tables))
    node = D.N("giqldisjoin", this=D.N("subquery", this=D.select([D.star()], D.tbl("features"), [])), reference=None)
    with pytest.raises(HipDeclined, match="DISJOIN over a sub-query"):
        lower_disjoin_statement(D.select([D.star()], node, []), node, D.ExpansionContext(tables))
    node = _disjoin_node("features")
    with pytest.raises(HipDeclined, match="WHERE over the rows of DISJOIN"):
        lower_disjoin_statement(D.select([D.star()], node, [], where=D.cmp("gt", D.col(None, "disjoin_start"), D.lit(5))),
                                node, D.ExpansionContext(tables))


def test_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "giql_hip.h")).read()
    L = _lib.load()
    for sym in ("giql_hip_disjoin_plan_dev", "giql_hip_disjoin_fill_dev"):
        assert re.search(rf"\bint {sym}\s*\(", header), sym
        assert sym in _lib.SYMBOLS and hasattr(L, sym)
        assert getattr(L, sym).argtypes is not None
    assert "disjoin.py:147-202" in header
    assert L.giql_hip_abi_version() >= 3


def test_brute_force_agrees_with_every_golden_case():
    cases = golden_cases()
    assert len(cases) >= 100 and sum(c["id"].startswith("known-") for c in cases) == 10
    assert {tuple(c["encoding"]) for c in cases} == set(OFFSETS)
    assert any(c["reference"] is None for c in cases) and any(c["reference"] for c in cases)
    for c in cases:
        assert brute_force(c["target"], c["reference"], c["encoding"]) == c["expected"], c["id"]


def test_vectorised_brute_force_agrees_with_every_golden_case():
    for c in golden_cases():
        so, eo = OFFSETS[tuple(c["encoding"])]
        names = sorted({r[0] for r in c["target"]} | {r[0] for r in c["reference"] or []})
        code = {n: i for i, n in enumerate(names)}
        t = np.array([[code[r[0]], r[1] + so, r[2] + eo] for r in c["target"]], np.int64).reshape(-1, 3)
        args = [t[:, 0], t[:, 1], t[:, 2]]
        if c["reference"] is not None:
            r = np.array([[code[x[0]], x[1], x[2]] for x in c["reference"]], np.int64).reshape(-1, 3)
            args += [r[:, 0], r[:, 1], r[:, 2]]
        got = brute_force_arrays(*args)
        got[:, 1] -= so
        got[:, 2] -= eo
        assert sorted(got.tolist()) == c["expected"], c["id"]
