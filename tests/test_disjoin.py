"""DISJOIN without a GPU: the front ends, the plan, the declines, the ABI, the brute-force restatement against the
golden fixture (tests/golden/disjoin.json, minted by tests/golden/make_disjoin.py), the vectorised brute force
against the row-by-row one, and the numpy mirror of the fill's tiles that shows which path each constructed case of
tests/test_disjoin_paths.py reaches."""

import os
import re

import numpy as np
import pytest

import _ast_doubles as D
import _disjoin_ref as R
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


# ---------------------------------------------------------------- the fast reference, anchored row by row
def _same(case):
    fast, slow = case.expected(), case.expected_row_by_row()
    assert fast.shape == slow.shape and np.array_equal(fast, slow), case.id


def test_vectorised_brute_force_equals_the_row_by_row_one_on_every_constructed_case():
    """brute_force_arrays has the kernel's own shape (breakpoints, depth, two searchsorted); brute_force does not.
    Only what passes here may serve the GPU tests as their truth (tests/test_disjoin_paths.py)."""
    paths = R.path_cases()
    for case, cnt in paths.values():
        _same(case)
        assert np.array_equal(case.counts(), cnt), case.id          # the builder gives the counts it was asked for
    cover = R.coverage_cases()
    assert len([c for c in cover if c.id.startswith("encodings-")]) == 16
    for case in cover:
        _same(case)
    assert len(paths) + len(cover) == 50


def test_vectorised_brute_force_equals_the_row_by_row_one_on_200_seeded_tables():
    seen = {"self": 0, "reference": 0, "negative": 0, "zero_t": 0, "zero_r": 0, "dup": 0, "book": 0, "one_side": 0,
            "rows": 0}
    for seed in range(200):
        case = R.seeded_small_case(seed)
        tc, ts, te = case.t
        assert 1 <= len(tc) <= 300 and (case.r is None or len(case.r[0]) <= 300)
        _same(case)
        rc, rs, re_ = case.r if case.r is not None else case.t
        seen["self" if case.r is None else "reference"] += 1
        seen["negative"] += int(ts.min() < 0 and (len(rs) == 0 or rs.min() < 0))
        seen["zero_t"] += int((ts == te).any())
        seen["zero_r"] += int((rs == re_).any())
        seen["dup"] += int(len({*zip(rc.tolist(), rs.tolist(), re_.tolist())}) < len(rc))
        seen["book"] += int(bool(set(zip(rc.tolist(), rs.tolist())) & set(zip(rc.tolist(), re_.tolist()))))
        seen["one_side"] += int(case.r is not None and set(tc.tolist()) != set(rc.tolist()))
        seen["rows"] += len(case.expected())
    assert seen["self"] == seen["reference"] == 100
    assert all(seen[k] >= 60 for k in ("negative", "zero_t", "zero_r", "dup", "book")) and seen["one_side"] >= 30, seen
    assert seen["rows"] > 20_000


# ---------------------------------------------------------------- every path case reaches the path it names
def test_fill_mirror_on_hand_counted_tiles():
    c = {"tile": 8, "items": 4, "off_cap": 3}
    t = R.fill_mirror([0, 3, 0, 0, 6, 0, 2, 0], consts=c)           # offsets 0 0 3 3 3 9 9 11, total 11
    assert [(x["k0"], x["k1"], x["r_lo"], x["nr"], x["staged"]) for x in t] == [(0, 8, 1, 4, False), (8, 11, 4, 3, True)]
    assert [(x["vec_quads"], x["scalar_quads"], x["partial"], x["k0_in_row"]) for x in t] == [(2, 0, False, 0),
                                                                                              (0, 1, True, 5)]
    assert [(x["zero_rows"], x["zero_after"]) for x in t] == [(2, 1), (1, 1)]
    assert all(x["vec_quads"] == 0 for x in R.fill_mirror([0, 3, 0, 0, 6, 0, 2, 0], align=(0, 4, 0), consts=c))
    assert [R.tiles_of_row([0, 3, 0, 0, 6, 0, 2, 0], r, consts=c) for r in (0, 1, 4, 6)] == [0, 1, 2, 1]


def test_every_path_case_reaches_its_path():
    """A retuned DJ_FILL_TILE / DJ_FILL_ITEMS / DJ_OFF_CAP must fail here, not quietly empty a GPU case."""
    k = R.fill_constants()
    tile, items, cap = k["tile"], k["items"], k["off_cap"]
    cases = R.path_cases()
    m = {cid: R.fill_mirror(cnt) for cid, (_case, cnt) in cases.items()}
    cnt = {cid: c for cid, (_case, c) in cases.items()}
    # the unstaged branch and both sides of its cap
    assert [(x["nr"], x["staged"]) for x in m["unstaged-5000"]] == [(5002, False)]
    assert [(x["nr"], x["staged"]) for x in m["cap-exactly"]] == [(cap, True)]
    assert [(x["nr"], x["staged"]) for x in m["cap-plus-one"]] == [(cap + 1, False)]
    x, = m["unstaged-leading-trailing-zeros"]
    assert not x["staged"] and x["r_lo"] == 9 and x["zero_after"] == 11 and cnt["unstaged-leading-trailing-zeros"][0] == 0
    z = m["zero-rows-at-tile-edges"]
    assert len(z) == 3 and all(x["staged"] and x["k0_in_row"] == 0 for x in z)
    assert [x["zero_after"] for x in z] == [7, 3, 2]      # zero-piece rows between a tile's last slot and the next's first
    assert z[1]["r_lo"] == 9 and z[2]["r_lo"] == 14       # ... skipped: the next tile opens on the row that owns its slot
    u = m["unstaged-second-tile"]
    assert [x["staged"] for x in u] == [True, False, True] and u[1]["k0_in_row"] == 0 and u[1]["zero_rows"] > cap
    # tile edges
    for total in (1, 3, 4, 5, tile - 1, tile, tile + 1, 4 * tile - 1, 4 * tile + 1):
        t = m[f"total-{total}"]
        assert len(t) == -(-total // tile) and t[-1]["k1"] == total
        assert t[-1]["partial"] == (total % items != 0)
        assert sum(x["vec_quads"] for x in t) == total // items
        assert all(x["staged"] for x in t)
    assert m["total-1"][0]["vec_quads"] == 0 and m["total-4"][0]["scalar_quads"] == 0
    assert [x["k0_in_row"] for x in m["parent-starts-at-tile-boundary"]] == [0, 0]
    assert m["parent-starts-at-tile-boundary"][1]["r_lo"] == 2
    assert [x["k0_in_row"] for x in m["parent-straddles-two-tiles"]] == [0, 10]          # 10 of the row's 30 pieces lie in the first tile
    assert R.tiles_of_row(cnt["parent-straddles-two-tiles"], 1) == 2
    assert R.tiles_of_row(cnt["parent-straddles-five-tiles"], 1) == 5
    assert [x["r_lo"] for x in m["parent-straddles-five-tiles"]] == [0, 1, 1, 1, 1]
    for mod in (1, 2, 3):
        t = m[f"total-mod-4-is-{mod}"]
        assert t[-1]["k1"] % items == mod and t[-1]["partial"] and t[-1]["scalar_quads"] == 1
    # unaligned outputs: no quad takes the 16-byte store, whichever of the three is off
    for align in ((4, 0, 0), (0, 4, 0), (0, 0, 4), (4, 4, 4)):
        t = R.fill_mirror(cnt["total-%d" % (4 * tile + 1)], align=align)
        assert sum(x["vec_quads"] for x in t) == 0 and sum(x["scalar_quads"] for x in t) == tile + 1
