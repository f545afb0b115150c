"""Column-to-column CONTAINS / WITHIN joins without a GPU: the golden fixture (tests/golden/contains_within.json,
minted by tests/golden/make_contains.py) against the numpy brute force, both front ends, the plan's serialisation,
every decline with its reason, the literal forms' residuals, and the ABI."""

import ctypes
import os
import re

import pytest

import _ast_doubles as A
import _contain_ref as R
from giql_amd import _lib, plugin
from giql_amd.plan import PLAN_PREFIX, JoinPlan
from giql_amd.shape import HipDeclined
from giql_amd.table import Table, build_tables
from giql_amd.transpile import build_plan, transpile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = ["genes", "variants"]


# ------------------------------------------------------------------ the fixture
def test_fixture_meets_its_conditions():
    cases = R.golden_cases()
    known = [c for c in cases if c["id"].startswith("known-")]
    seeded = [c for c in cases if c["id"].startswith("random-")]
    assert [c["source"] for c in known] == ["tests/integration/bedtools/test_contains.py:57",
                                            "tests/integration/bedtools/test_within.py:58"]
    assert len(seeded) >= 100
    assert all(len(c["a"]) < 200 and len(c["b"]) < 200 for c in seeded)
    assert sum(not c["contains"] for c in seeded) <= len(seeded) // 10
    assert 2 * sum(c["loose_overlaps"] > 0 for c in seeded) >= len(seeded)
    assert {(tuple(c["enc_a"]), tuple(c["enc_b"])) for c in seeded} == {(x, y) for x in R.OFFSETS for y in R.OFFSETS}
    assert {len({r[0] for r in c["a"] + c["b"]}) for c in seeded} == {1, 2, 3, 4}
    tags = {t for c in seeded for t in c["tags"]}
    assert {"absent-chrom", "irregular-outer", "irregular-inner", "uniform-inner-L1", "outer-shorter-than-L"} <= tags
    assert any(t.startswith("uniform-inner-L") and t != "uniform-inner-L1" for t in tags)


def test_brute_force_reproduces_the_fixture():
    for c in R.golden_cases():
        assert R.case_brute_force(c, "contains") == c["contains"], c["id"]
        assert R.case_brute_force(c, "within") == c["within"], c["id"]


def test_known_answers_as_upstream_states_them():
    by_id = {c["id"]: c for c in R.golden_cases()}
    assert by_id["known-test_contains.py:57"]["contains"] == [[0, 0], [0, 1], [1, 1]]
    assert by_id["known-test_within.py:58"]["within"] == [[0, 0]]


# ------------------------------------------------------------------ the front ends
@pytest.mark.parametrize("word", ["CONTAINS", "WITHIN"])
def test_the_mirror_lowers_the_join_to_an_inner_plan(word):
    # (declined with "CONTAINS predicate" before the operator had a device path)
    text = transpile(f"SELECT a.name, b.name FROM genes a JOIN variants b ON a.interval {word} b.interval", TABLES,
                     dialect="hip")
    assert text.startswith(PLAN_PREFIX)
    plan = JoinPlan.from_string(text)
    assert plan.kind == "INNER" and plan.predicate == word.lower()
    assert (plan.left.table, plan.right.table) == ("genes", "variants") and not plan.residuals


def test_where_form_operand_order_and_residuals():
    # upstream's quick start: FROM a, b WHERE a.interval CONTAINS b.interval
    plan = build_plan("SELECT a.name, b.name FROM genes a, variants b WHERE a.interval CONTAINS b.interval", TABLES)
    assert plan.kind == "INNER" and plan.predicate == "contains"
    # the plan states the predicate as left <predicate> right: operands written the other way round flip it
    plan = build_plan("SELECT a.name FROM genes a JOIN variants b ON b.interval WITHIN a.interval", TABLES)
    assert plan.predicate == "contains" and plan.left.table == "genes"
    plan = build_plan("SELECT a.name FROM genes a JOIN variants b ON b.interval CONTAINS a.interval", TABLES)
    assert plan.predicate == "within"
    plan = build_plan("SELECT a.name FROM genes a JOIN variants b ON a.interval CONTAINS b.interval AND a.score > 5 "
                      "AND (a.start < b.start OR b.name = 'x') WHERE b.strand = '+' ORDER BY a.start LIMIT 3", TABLES)
    assert plan.predicate == "contains" and plan.limit == 3
    assert [(r.clause, r.op, r.group) for r in plan.residuals] == [("on", ">", 0), ("on", "<", 1), ("on", "=", 1),
                                                                    ("where", "=", 0)]


def _spatial(key, l=("a", "interval"), r=("b", "interval")):
    return A.N(key, this=A.col(*l), expression=A.col(*r))


def _run_plugin(root, node, key, tables=("genes", "variants")):
    tbls = build_tables(list(tables))
    cols = {arg: A.resolved(node.args[arg].args["table"].args["this"], None) for arg in ("this", "expression")}
    ctx = A.ExpansionContext(tables=tbls, resolution=A.OperatorResolution(operator=key.title(), columns=cols))
    calls = []
    expander = plugin.make_expander(lambda n, c: calls.append(n) or "FALLBACK", lambda payload: ("COMMAND", payload), key)
    return expander(node, ctx), ctx, calls


@pytest.mark.parametrize("key", ["contains", "within"])
def test_the_plugin_lowers_to_the_same_plan_as_the_mirror(key):
    node = _spatial(key)
    root = A.select([A.col("a", "name"), A.alias(A.col("b", "name"), "v")], A.tbl("genes", "a"),
                    [A.join(A.tbl("variants", "b"), on=A.conj(node, A.cmp("gt", A.col("a", "score"), A.lit(5))))])
    out, ctx, calls = _run_plugin(root, node, key)
    assert out is node and not calls and len(ctx.finalizers) == 1
    tag, payload = ctx.finalizers[0](root)
    assert tag == "COMMAND"
    want = build_plan(f"SELECT a.name, b.name AS v FROM genes a JOIN variants b ON a.interval {key.upper()} b.interval "
                      "AND a.score > 5", TABLES)
    assert JoinPlan.from_string(payload) == want and want.predicate == key


def test_the_plugin_falls_back_like_the_intersects_expander():
    # the Contains expander only takes Contains nodes; a literal operand, a sibling spatial predicate and a
    # declined shape all go to the generic expansion
    node = _spatial("within")
    root = A.select([A.col("a", "name")], A.tbl("genes", "a"), [A.join(A.tbl("variants", "b"), on=node)])
    out, ctx, calls = _run_plugin(root, node, "contains")
    assert out == "FALLBACK" and calls == [node] and not ctx.finalizers
    lit = A.N("contains", this=A.col(None, "interval"), expression=A.lit("chr1:100-200"))
    root = A.select([A.star()], A.tbl("genes"), [], where=lit)
    tbls = build_tables(["genes"])
    ctx = A.ExpansionContext(tables=tbls, resolution=A.OperatorResolution())
    expander = plugin.make_expander(lambda n, c: "FALLBACK", lambda p: p, "contains")
    assert expander(lit, ctx) == "FALLBACK" and not ctx.finalizers
    node = _spatial("contains")
    other = _spatial("intersects")
    root = A.select([A.col("a", "name")], A.tbl("genes", "a"), [A.join(A.tbl("variants", "b"), on=A.conj(node, other))])
    out, ctx, calls = _run_plugin(root, node, "contains")
    assert out == "FALLBACK" and not ctx.finalizers
    node = _spatial("contains")
    root = A.select([A.col("a", "name")], A.tbl("genes", "a"), [A.join(A.tbl("variants", "b"), on=node, kind="SEMI")])
    out, ctx, calls = _run_plugin(root, node, "contains")
    assert out == "FALLBACK" and not ctx.finalizers


# ------------------------------------------------------------------ the plan
def test_plan_round_trips_and_old_strings_load_as_intersects():
    plan = build_plan("SELECT a.name FROM genes a JOIN variants b ON a.interval WITHIN b.interval WHERE a.score > 1", TABLES)
    assert plan.to_dict()["predicate"] == "within"
    assert JoinPlan.from_string(plan.to_string()) == plan and JoinPlan.from_dict(plan.to_dict()) == plan
    old = build_plan("SELECT a.name FROM genes a JOIN variants b ON a.interval INTERSECTS b.interval", TABLES)
    d = old.to_dict()
    assert d.pop("predicate") == "intersects"
    import json
    loaded = JoinPlan.from_string(PLAN_PREFIX + json.dumps(d, sort_keys=True, separators=(",", ":")))
    assert loaded == old and loaded.predicate == "intersects"
    with pytest.raises(ValueError, match="unknown join predicate"):
        JoinPlan("INNER", old.left, old.right, predicate="overlaps")
    with pytest.raises(ValueError, match="needs an INNER plan"):
        JoinPlan("SEMI", old.left, old.right, predicate="contains")


# ------------------------------------------------------------------ what declines
@pytest.mark.parametrize("query, reason", [
    ("SELECT a.name FROM genes a JOIN variants b ON a.interval CONTAINS b.interval AND a.interval INTERSECTS b.interval",
     "more than one spatial predicate in a join"),
    ("SELECT a.name FROM genes a JOIN variants b ON a.interval CONTAINS b.interval AND b.interval WITHIN a.interval",
     "more than one spatial predicate in a join"),
    ("SELECT a.name FROM genes a SEMI JOIN variants b ON a.interval CONTAINS b.interval", "SEMI join over CONTAINS"),
    ("SELECT a.name FROM genes a ANTI JOIN variants b ON a.interval WITHIN b.interval", "ANTI join over WITHIN"),
    ("SELECT a.chrom, a.start, a.end, COUNT(b.start) FROM genes a LEFT JOIN variants b ON a.interval CONTAINS b.interval "
     "GROUP BY a.chrom, a.start, a.end", "count_overlaps over CONTAINS"),
    ("SELECT a.name FROM genes a JOIN variants b ON NOT a.interval CONTAINS b.interval", "NOT over a spatial predicate"),
    ("SELECT a.name FROM genes a JOIN variants b ON a.interval WITHIN b.interval OR a.score > 5",
     "spatial predicate under OR"),
    ("SELECT a.name FROM genes a JOIN genes b ON a.interval CONTAINS b.interval", "self-join"),
    ("SELECT a.name FROM genes a JOIN variants b ON a.interval CONTAINS ANY('chr1:1-2', 'chr1:5-9')", "CONTAINS ANY/ALL"),
    ("SELECT a.name FROM genes a JOIN variants b ON a.interval WITHIN 'chr1:100-200'", "literal-range WITHIN inside a join"),
    ("SELECT * FROM genes WHERE interval CONTAINS 'chr1:150'", "literal range formats other than 'chr:start-end'"),
    ("SELECT * FROM genes WHERE interval WITHIN ALL('chr1:1-2', 'chr1:5-9')", "no join (a single-table predicate)"),
])
def test_declines_with_a_reason(query, reason):
    with pytest.raises(HipDeclined, match=re.escape(reason)):
        transpile(query, TABLES, dialect="hip")


def test_two_intersects_keep_their_reason():
    with pytest.raises(HipDeclined, match="more than one INTERSECTS"):
        transpile("SELECT a.name FROM genes a JOIN variants b ON a.interval INTERSECTS b.interval "
                  "AND b.interval INTERSECTS a.interval", TABLES, dialect="hip")


# ------------------------------------------------------------------ the literal forms
@pytest.mark.parametrize("word, want", [
    ("CONTAINS", [("chrom", "=", "chr1"), ("start", "<=", 100), ("end", ">=", 200)]),
    ("WITHIN", [("chrom", "=", "chr1"), ("start", ">=", 100), ("end", "<=", 200)]),
    ("INTERSECTS", [("chrom", "=", "chr1"), ("start", "<", 200), ("end", ">", 100)]),
])
def test_literal_forms_lower_to_three_residuals(word, want):
    plan = build_plan(f"SELECT name FROM genes WHERE interval {word} 'chr1:100-200' AND score > 3", ["genes"])
    assert plan.kind == "FILTER" and plan.right is None and plan.predicate == "intersects"
    got = [(r.lhs.value, r.op, r.rhs.value) for r in plan.residuals]
    assert got == want + [("score", ">", 3)]


def test_literal_forms_keep_the_restrictions_of_the_literal_intersects():
    with pytest.raises(HipDeclined, match="non-canonical table"):
        build_plan("SELECT * FROM genes WHERE interval WITHIN 'chr1:100-200'",
                   [Table("genes", coordinate_system="1based", interval_type="closed")])
    with pytest.raises(ValueError, match="Start must be less than end"):
        build_plan("SELECT * FROM genes WHERE interval CONTAINS 'chr1:200-100'", ["genes"])
    with pytest.raises(HipDeclined, match="more than one spatial predicate"):
        build_plan("SELECT * FROM genes WHERE interval CONTAINS 'chr1:1-5' AND interval WITHIN 'chr1:0-9'", ["genes"])


# ------------------------------------------------------------------ the ABI
def test_abi_version_symbols_and_header():
    header = open(os.path.join(ROOT, "include", "giql_hip.h")).read()
    L = _lib.load()
    assert L.giql_hip_abi_version() == 4
    assert re.search(r"#define GIQL_HIP_ABI_VERSION 4\b", header)
    for sym in ("giql_hip_contain_plan_dev", "giql_hip_contain_fill_dev"):
        assert re.search(rf"\bint {sym}\s*\(", header), sym
        assert sym in _lib.SYMBOLS and hasattr(L, sym)
        assert getattr(L, sym).argtypes is not None
    assert "intersects.py:155-166" in header


def test_null_arguments_are_refused_before_any_device_work():
    L = _lib.load()
    n = ctypes.c_int64(-1)
    side = _lib.CSide()
    assert L.giql_hip_contain_plan_dev(None, ctypes.byref(side), ctypes.byref(side), 1, None,
                                       ctypes.byref(n)) == _lib.GIQL_ERR_INVALID
    assert L.giql_hip_contain_fill_dev(None, None, None, 0, None) == _lib.GIQL_ERR_INVALID
    with pytest.raises(_lib.GiqlHipError) as exc:
        _lib.check(L.giql_hip_contain_fill_dev(None, None, None, 0, None))
    assert exc.value.code == _lib.GIQL_ERR_INVALID and "ctx is NULL" in str(exc.value)


# ------------------------------------------------------------------ the candidate tiles, mirrored in numpy
def _mirror_general_form(outer, inner, tile, qcap, n_waves, win):
    """The general form's index arithmetic restated in numpy: ``_contain_ref.mirror_general_form`` (candidate ranges,
    u64 offsets, ``k_partition``, the staged row records, the per-wave walk -- the first window's search, the ``k + 1``
    test, the search from ``k + 2`` -- and the search of the offsets for a tile past the stage).  Returns the pairs in
    slot order, the number of tiles that took the search outside the stage, and the per-tile records (row count,
    staged or not, owners per window) the path tests assert reach with."""
    pairs, info = R.mirror_general_form(outer, inner, tile, qcap, n_waves, win)
    assert all(t["staged"] == (t["nqt"] <= qcap) and t["owners"].size == -(-t["tile_len"] // win) for t in info)
    return pairs, sum(not t["staged"] for t in info), info


@pytest.mark.parametrize("tile, qcap, n_waves, win", [(64, 16, 4, 4), (7, 2, 1, 1), (16384, 4096, 16, 64)],
                         ids=["64-16", "7-2", "16384-4096"])
def test_numpy_mirror_of_the_candidate_tiles_matches_the_brute_force(tile, qcap, n_waves, win):
    import numpy as np

    r = np.random.default_rng(tile)
    n_o, n_i = 300, 900
    os_ = np.concatenate([[0, 0], r.integers(0, 5000, n_o - 2)])
    oe = np.concatenate([[6000, 5000], os_[2:] + r.integers(1, 400, n_o - 2)])      # two rows that own most candidates
    os_[100:160] = 5500 + np.arange(60)                                              # a run of rows without candidates
    oe[100:160] = os_[100:160] + 1
    is_ = r.integers(0, 5000, n_i)
    ie = is_ + r.integers(1, 200, n_i)
    got, unstaged, info = _mirror_general_form((os_, oe), (is_, ie), tile, qcap, n_waves, win)
    zeros = np.zeros
    want = R.contain_pairs(zeros(n_o, np.int64), os_, oe, zeros(n_i, np.int64), is_, ie)
    assert np.array_equal(R.sort_pairs(got), want) and want.shape[0] > 1000
    assert (unstaged > 0) == (qcap < 60)
    # the walk met windows with one owner and windows in which the owner changes
    owners = np.concatenate([t["owners"] for t in info if t["staged"]])
    assert owners.min() == 1 and (owners.max() > 1 or win == 1)


@pytest.mark.parametrize("cid", list(R.PATH_CASES))
def test_every_path_case_reaches_its_path(cid):
    """Each generator of tests/test_contain_paths.py, without a GPU: the mirror equals the brute force on it and shows
    the path the case is named after (``_contain_ref.reach`` holds the assertions, the GPU tests call it too)."""
    ev = R.reach(cid)
    print(f"\n[{cid}] " + ", ".join(f"{k}={v}" for k, v in ev.items()))


def test_sort_based_reference_equals_the_brute_force_on_seeded_tables():
    """``contain_pairs_sorted`` (the truth of the cases the brute force would take minutes on) against
    ``contain_pairs``: 240 seeded tables -- one to four chromosomes, zero-length and inverted rows on either side,
    negative coordinates, duplicated rows -- and every fixture case, which covers the four encodings on both sides."""
    import numpy as np

    odd = 0
    for seed in range(240):
        r = np.random.default_rng(seed)
        nch, n_o, n_i = 1 + seed % 4, int(r.integers(1, 250)), int(r.integers(1, 250))
        lo = -500 if seed % 5 == 0 else 0
        oc, ic = r.integers(0, nch, n_o), r.integers(0, nch, n_i)
        os_, is_ = lo + r.integers(0, 1000, n_o), lo + r.integers(0, 1000, n_i)
        oe, ie = os_ + r.integers(1, 300, n_o), is_ + r.integers(1, 80, n_i)
        if seed % 3:                                     # irregular rows, and [p, p) inside [p, p)
            for s, e in ((os_, oe), (is_, ie)):
                bad = r.random(s.size) < 0.1
                e[bad] = s[bad] - r.integers(0, 20, int(bad.sum()))
            k = min(n_o, n_i, 5)
            ic[:k], is_[:k], ie[:k] = oc[:k], os_[:k], np.minimum(oe[:k], os_[:k])
            odd += int((oe <= os_).sum() > 0 and (ie <= is_).sum() > 0)
        want = R.contain_pairs(oc, os_, oe, ic, is_, ie)
        assert np.array_equal(R.contain_pairs_sorted(oc, os_, oe, ic, is_, ie), want), seed
    assert odd >= 100
    encodings = set()
    for c in R.golden_cases():
        ac, as_, ae, (aso, aeo), bc, bs, be, (bso, beo), _ = R.case_arrays(c)
        a = (ac, as_.astype(np.int64) + aso, ae.astype(np.int64) + aeo)
        b = (bc, bs.astype(np.int64) + bso, be.astype(np.int64) + beo)
        assert R.contain_pairs_sorted(*a, *b).tolist() == c["contains"], c["id"]
        encodings.add((tuple(c["enc_a"]), tuple(c["enc_b"])))
    assert len(encodings) == 16
