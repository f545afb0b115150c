"""Aggregates over an expression of a join's pair (the ``aggregate_expressions`` opt-in beside ``join_aggregates``;
"Overlap Statistics", docs/recipes/advanced.rst) without a GPU: the reference against sqlite-minted rows, the plans
and declines of the text front end, that nothing changes without both flags, execute()'s routing, the integer
overflow bound, the host fold of a LEFT join's unmatched rows, and the C ABI's declaration.  The GPU halves are
tests/test_pair_expr_agg_gpu.py (the kernel and its entry point) and tests/test_aggregate_expressions_gpu.py."""
import ctypes
import inspect
import json
import os
import re
import shutil
import subprocess
from dataclasses import replace

import numpy as np
import pytest

import _agg_expr_queries as Q
import _pair_expr_agg_ref as R
from giql_amd import _lib
from giql_amd import execute as X
from giql_amd.plan import Aggregate, JoinPlan, Operand, Residual
from giql_amd.shape import HipDeclined
from giql_amd.transpile import build_plan, transpile

pa = pytest.importorskip("pyarrow")

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = json.load(open(os.path.join(HERE, "golden", "aggregate_expressions.json")))
RECORDED = json.load(open(os.path.join(HERE, "golden", "aggregate_expressions_plans.json")))
BOTH = {"join_aggregates": True, "aggregate_expressions": True}


# ---------------------------------------------------------------- the reference against sqlite
@pytest.mark.parametrize("case", GOLDEN["cases"], ids=lambda c: c["name"])
def test_the_reference_answers_the_golden_rows(case):
    a, b = R.golden_tables(GOLDEN)
    aggs = [(f, name) for name in GOLDEN["expressions"] for f in GOLDEN["functions"]]
    assert R.query_rows(a, b, case["join"], case["keys"], aggs, R.golden_trees(a, b)) == case["rows"]


def test_the_golden_holds_the_cases_it_exists_for():
    rows = next(c for c in GOLDEN["cases"] if c["name"] == "left_interval")["rows"]
    n = len(GOLDEN["functions"])
    col = {name: 4 + j * n for j, name in enumerate(GOLDEN["expressions"])}       # COUNT; + 1: SUM
    unmatched = [r for r in rows if r[3] == 1 and r[col["reach"]] == 0]
    assert unmatched
    for r in unmatched:     # the padded row: LEAST / GREATEST skip the NULLs, the CASE answers 0, b.end - a.start is NULL
        assert r[col["overlap_bp"] + 1] == r[2] - r[1] and r[col["overlap_case"] + 1] == 0
        assert (r[col["overlap_case"]], r[col["reach"] + 1], r[col["weighted"] + 1]) == (1, None, None)
    assert any(r[col["reach"]] >= 1 and r[col["weighted"]] == 0 and r[col["weighted"] + 1] is None for r in rows)
    assert os.path.getsize(os.path.join(HERE, "golden", "aggregate_expressions.json")) <= \
        os.path.getsize(os.path.join(HERE, "golden", "join_aggregates.json"))


# ---------------------------------------------------------------- without both flags nothing changes
def test_the_fixture_holds_exactly_the_queries_of_the_list():
    assert sorted(RECORDED["cases"]) == sorted(Q.ALL) and len(RECORDED["recorded_at_commit"]) == 40
    assert len(Q.ALL) == len(Q.IN_SHAPE) + len(Q.DECLINES) + len(Q.NEIGHBOURS)
    for rec in RECORDED["cases"].values():
        assert sorted(rec) == sorted(Q.OPTIONS)
    assert "aggregate_expressions" not in json.dumps(RECORDED) and '\\"side\\":\\"x\\"' not in json.dumps(RECORDED)


@pytest.mark.parametrize("name", sorted(Q.ALL))
@pytest.mark.parametrize("opt", sorted(Q.OPTIONS))
def test_without_both_flags_every_query_lowers_as_recorded(name, opt):
    """The same text and the same exception type as at the recorded commit: with the new flag absent, False, and --
    where ``join_aggregates`` is not set -- True."""
    want, kw = RECORDED["cases"][name][opt], Q.OPTIONS[opt]
    assert Q.outcome(build_plan, Q.ALL[name], **kw) == want
    assert Q.outcome(build_plan, Q.ALL[name], aggregate_expressions=False, **kw) == want
    if not kw.get("join_aggregates"):
        assert Q.outcome(build_plan, Q.ALL[name], aggregate_expressions=True, **kw) == want
    if "plan" in want:
        assert transpile(Q.ALL[name], Q.TABLES, dialect="hip", **kw) == want["plan"]
        assert not any(a.side == "x" for a in JoinPlan.from_string(want["plan"]).aggregates)


@pytest.mark.parametrize("name", sorted(Q.IN_SHAPE) + sorted(Q.DECLINES))
def test_at_the_recorded_commit_every_such_query_declined_or_failed(name):
    """What the feature is for: none of these lowered under any of the older opt-ins."""
    assert all("plan" not in RECORDED["cases"][name][opt] for opt in Q.OPTIONS) or name == "parenthesised_column"


def test_select_expressions_alone_still_declines_an_aggregate_over_an_expression():
    for extra in ({}, {"aggregate_expressions": True}):
        with pytest.raises(HipDeclined, match="^aggregate over an expression:"):
            build_plan(Q.IN_SHAPE["overlap_statistics"], Q.TABLES, select_expressions=True, **extra)


@pytest.mark.parametrize("name", sorted(Q.NEIGHBOURS))
def test_a_query_without_such_an_aggregate_lowers_as_under_join_aggregates_alone(name):
    for opt, kw in Q.OPTIONS.items():
        if kw.get("join_aggregates"):
            assert Q.outcome(build_plan, Q.NEIGHBOURS[name], aggregate_expressions=True, **kw) == RECORDED["cases"][name][opt]


# ---------------------------------------------------------------- with both flags: plans
def _plan(name, **kw):
    return build_plan(Q.IN_SHAPE[name], Q.TABLES, **BOTH, **kw)


OVERLAP = ["fn", "-", [["fn", "least", [["l", "end"], ["r", "end"]]], ["fn", "greatest", [["l", "start"], ["r", "start"]]]]]


def test_the_overlap_statistics_plan():
    plan = _plan("overlap_statistics")
    assert plan.kind == "INNER" and plan.join_aggregates and plan.group_by == ("chrom",)
    assert plan.aggregates == (Aggregate("COUNT", "*", "*", "overlap_count"), Aggregate("AVG", "x", "0", "avg_overlap_bp"),
                               Aggregate("SUM", "x", "0", "total_overlap_bp"))
    assert [(e.kind, e.value) for e in plan.expressions] == [("expr", OVERLAP)]      # the same tree once
    assert plan.order_by == (("chrom", False, True),) and plan.output == ("chrom", "overlap_count", "avg_overlap_bp", "total_overlap_bp")
    assert [p.side for p in plan.projection] == ["l"]                                # no projection names an expression


def test_the_plans_of_the_other_forms():
    left = _plan("left_case")
    assert left.kind == "LEFT" and [(a.func, a.side, a.column) for a in left.aggregates] == [("SUM", "x", "0"), ("COUNT", "x", "0")]
    assert left.expressions[0].value[:2] == ["fn", "if"] and left.expressions[0].value[2][1] == ["int", 0]
    twice = _plan("same_tree_twice")
    assert [(a.func, a.column) for a in twice.aggregates] == [("SUM", "0"), ("MAX", "0"), ("SUM", "1")] and len(twice.expressions) == 2
    mixed = _plan("weighted")
    assert [(a.func, a.side, a.column) for a in mixed.aggregates] == [("SUM", "x", "0"), ("AVG", "r", "score")]
    assert mixed.expressions[0].value == ["fn", "*", [["r", "score"], OVERLAP]]
    # a parenthesised plain column is the column aggregate it always was
    assert _plan("parenthesised_column").aggregates == (Aggregate("SUM", "r", "score", "s"),) and not _plan("parenthesised_column").expressions
    assert _plan("unary_minus").expressions[0].value == ["fn", "neg", [["r", "score"]]]
    tail = _plan("tail_on_the_alias")
    assert tail.having and tail.order_by == (("bp", True, False),) and tail.limit == 3 and len(tail.residuals) == 1
    assert _plan("contains").predicate == "contains"
    # LEFT needs no outer_joins, and the other opt-ins do not disturb the shape
    assert _plan("left_covered_bp") == _plan("left_covered_bp", outer_joins=True, select_expressions=True)


@pytest.mark.parametrize("name", sorted(Q.IN_SHAPE))
def test_the_text_form_round_trips(name):
    plan = _plan(name)
    text = transpile(Q.IN_SHAPE[name], Q.TABLES, dialect="hip", **BOTH)
    assert text == plan.to_string() and JoinPlan.from_string(text) == plan and JoinPlan.from_string(text).to_string() == text
    assert plan.join_aggregates


@pytest.mark.parametrize("name", sorted(Q.DECLINES))
def test_the_declines_each_with_its_own_text(name):
    query, text = Q.DECLINES[name]
    with pytest.raises(HipDeclined) as err:
        build_plan(query, Q.TABLES, **BOTH)
    assert str(err.value).startswith(text), str(err.value)


def test_the_decline_texts_are_distinct_per_case():
    texts = {Q.DECLINES[n][1] for n in ("distinct", "constant", "string_valued", "comparison", "distance_inside", "in_having",
                                        "in_order_by", "right_side_key")}
    assert len(texts) == 8 and not any(t == "aggregate over an expression" for t in texts)


def test_the_plugin_front_end_carries_no_opt_in():
    from giql_amd import plugin

    text = inspect.getsource(plugin)
    assert "aggregate_expressions" not in text and 'decline("aggregate over an expression")' in text


def test_the_index_of_an_expression_is_checked():
    plan = _plan("same_tree_twice")
    for bad in (dict(expressions=plan.expressions[:1]), dict(join_aggregates=False),
                dict(aggregates=(Aggregate("SUM", "x", "two", "s"),))):
        with pytest.raises(ValueError, match="names expression|join_aggregates"):
            replace(plan, **bad)


def test_the_flag_reaches_every_entry_point():
    for fn in (build_plan, transpile, X.execute):
        p = inspect.signature(fn).parameters["aggregate_expressions"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY


# ---------------------------------------------------------------- execute(): routing
def test_execute_routes_expressions_that_only_aggregates_refer_to():
    route = X._routes_join_aggregates
    types = {"score": pa.float64()}
    for name in ("overlap_statistics", "left_case", "weighted", "same_tree_twice"):
        plan = _plan(name)
        assert route(plan, types, False, None) and route(plan, types, False, [0]), name
        assert not route(plan, types, True, None) and not route(plan, types, False, [0, 1]), name
    mixed = _plan("weighted")
    assert not route(mixed, {"score": pa.string()}, False, None)                 # its column aggregate still needs a number
    assert route(_plan("overlap_statistics"), {}, False, None)                   # an expression needs no right type here
    twice = _plan("same_tree_twice")
    # an expression no aggregate names (a computed column's), or an aggregate past the expressions: not this path
    extra = replace(twice, expressions=twice.expressions + twice.expressions[:1])
    assert not route(extra, types, False, None)
    where = _plan("tail_on_the_alias")
    assert route(where, types, False, None)
    left = _plan("left_case")
    moved = replace(left, residuals=(Residual("where", Operand("l", "score"), ">", Operand("int", 3)),))
    assert not route(moved, types, False, None)


# ---------------------------------------------------------------- the interval bound of an integer SUM / AVG
def _info(bounds, floats=()):
    return lambda side, column: (bounds.get((side, column), 0), (side, column) in floats)


def test_the_bound_adds_multiplies_and_takes_the_largest_argument():
    bound = X.expression_abs_bound
    info = _info({("l", "start"): 1000, ("l", "end"): 1100, ("r", "start"): 5000, ("r", "end"): 5100, ("r", "w"): 7})
    assert bound(["l", "end"], info) == 1100 and bound(["int", -12], info) == 12
    assert bound(OVERLAP, info) == 5100 + 5000                                   # max(1100, 5100) + max(1000, 5000)
    assert bound(["fn", "*", [["r", "w"], OVERLAP]], info) == 7 * 10100
    assert bound(["fn", "*", [["r", "w"], ["r", "w"], ["int", 3]]], info) == 147
    assert bound(["fn", "neg", [OVERLAP]], info) == 10100 and bound(["fn", "abs", [["fn", "-", [["l", "start"], ["r", "w"]]]]], info) == 1007
    case = ["fn", "if", [["fn", ">", [["r", "end"], ["int", 10**12]]], ["int", 0], ["fn", "least", [OVERLAP, ["fn", "+", [["r", "w"], ["int", 1]]]]]]]
    assert bound(case, info) == 10100                                             # the condition's literal does not count
    assert bound(["fn", "if", [["fn", "isnull", [["r", "w"]]], ["fn", "null", []], ["r", "w"]]], info) == 7
    assert bound(["fn", "+", [["fn", "<", [["l", "start"], ["r", "start"]]], ["fn", "isnull", [["r", "w"]]]]], info) == 2


def test_a_tree_that_can_be_float_is_exempt():
    bound = X.expression_abs_bound
    info = _info({("r", "w"): 2**62, ("r", "score"): 0}, floats={("r", "score")})
    assert bound(["fn", "*", [["r", "w"], ["r", "w"]]], info) == 2**124
    for tree in (["fn", "/", [["r", "w"], ["int", 2]]], ["fn", "*", [["r", "w"], ["float", 1.0]]],
                 ["fn", "+", [["r", "w"], ["r", "score"]]], ["fn", "if", [["fn", "isnull", [["r", "w"]]], ["r", "score"], ["r", "w"]]],
                 ["fn", "greatest", [["r", "w"], ["fn", "neg", [["r", "score"]]]]]):
        assert bound(tree, info) is None, tree
        X.check_pair_expr_int_sum("s", tree, info, 2**62)
    # a float under a comparison leaves the tree an integer
    assert bound(["fn", "*", [["fn", ">", [["r", "score"], ["float", 0.5]]], ["r", "w"]]], info) == 2**62


def test_the_2_pow_63_edge_on_both_sides():
    info = _info({("r", "w"): 2**20, ("l", "v"): 2**21})
    tree = ["fn", "*", [["r", "w"], ["l", "v"]]]                                  # bound 2^41
    X.check_pair_expr_int_sum("total", tree, info, 2**22 - 1)                     # (2^22 - 1) * 2^41 < 2^63
    with pytest.raises(ValueError, match=r"aggregate 'total': 4194304 values of magnitude up to 2199023255552 can overflow"):
        X.check_pair_expr_int_sum("total", tree, info, 2**22)                     # 2^63: could wrap
    X.check_pair_expr_int_sum("total", ["fn", "-", [["r", "w"], ["r", "w"]]], info, 2**41)        # 2^41 * 2^21 = 2^62
    with pytest.raises(ValueError, match="aggregate 'total'"):
        X.check_pair_expr_int_sum("total", ["fn", "-", [["r", "w"], ["r", "w"]]], info, 2**42)
    X.check_pair_expr_int_sum("total", ["int", 0], info, 2**70)                   # a bound of 0 never overflows


def test_the_bound_reads_the_tables_min_and_max():
    lt = pa.table({"start": pa.array([5, -90, None], pa.int32()), "score": pa.array([1.5, None, 2.0]), "name": ["x", "y", None],
                   "flag": [True, False, None]})
    info = X._column_info(X._Residuals(_plan("left_only_tree"), lt, lt, None))
    assert info("l", "start") == (90, False) and info("r", "score") == (0, True) and info("l", "name") == (0, False)
    assert info("l", "flag") == (1, False)
    empty = pa.table({"start": pa.array([None, None], pa.int64())})
    assert X._column_info(X._Residuals(_plan("left_only_tree"), empty, empty, None))("l", "start") == (0, False)


# ---------------------------------------------------------------- the host fold and combine of a LEFT join's unmatched rows
def test_unmatched_left_rows_fold_in_as_partials_of_one_input():
    """Five left rows, two keys; rows 1 and 4 have no pair.  Expression 0 is overlap_bp (the padded row's value is
    a.end - a.start), expression 1 is b.end - a.start (NULL on the padded row)."""
    plan = build_plan("SELECT a.name, SUM(LEAST(a.end, b.end) - GREATEST(a.start, b.start)) AS bp, "
                      "AVG(LEAST(a.end, b.end) - GREATEST(a.start, b.start)) AS mean, COUNT(b.end - a.start) AS n, "
                      "MAX(b.end - a.start) AS hi, COUNT(*) AS c FROM a LEFT JOIN b ON a.interval INTERSECTS b.interval "
                      "GROUP BY a.name", Q.TABLES, **BOTH)
    assert [(a.func, a.column) for a in plan.aggregates] == [("SUM", "0"), ("AVG", "0"), ("COUNT", "1"), ("MAX", "1"), ("COUNT", "*")]
    pairs = np.array([2, 0, 1, 3, 0], np.int64)
    i64 = lambda *v: np.array(v, np.int64)   # noqa: E731
    partials = {("SUM", "__giql_x0"): (i64(30, 0, 7, 12, 0), i64(2, 0, 1, 3, 0)),
                ("COUNT", "__giql_x1"): (i64(2, 0, 1, 3, 0), i64(2, 0, 1, 3, 0)),
                ("MAX", "__giql_x1"): (i64(90, 0, 40, 55, 0), i64(2, 0, 1, 3, 0))}
    rows = np.array([1, 4], np.int32)
    padded = {"__giql_x0": (i64(100, 25), None), "__giql_x1": (i64(0, 0), np.array([0, 0], np.uint8))}
    folded = X._fold_padded_values(partials, padded, rows)
    assert folded[("SUM", "__giql_x0")][0].tolist() == [30, 100, 7, 12, 25] and folded[("SUM", "__giql_x0")][1].tolist() == [2, 1, 1, 3, 1]
    assert folded[("COUNT", "__giql_x1")][1].tolist() == [2, 0, 1, 3, 0] and folded[("MAX", "__giql_x1")][0].tolist() == [90, 0, 40, 55, 0]
    assert partials[("SUM", "__giql_x0")][0].tolist() == [30, 0, 7, 12, 0]                       # the input is left alone
    combine = replace(plan, expressions=(), aggregates=tuple(
        replace(a, side="r", column="__giql_x" + a.column) if a.side == "x" else a for a in plan.aggregates))
    lt = {"name": np.array(["k1", "k1", "k2", "k2", "k3"], object)}
    out = X._combine_join_partials(combine, lt, pairs, folded, {"__giql_x0": pa.int64(), "__giql_x1": pa.int64()})
    got = {r["name"]: r for r in out.to_pylist()}
    assert got["k1"] == {"name": "k1", "bp": 130, "mean": 130 / 3, "n": 2, "hi": 90, "c": 3}
    assert got["k2"] == {"name": "k2", "bp": 19, "mean": 19 / 4, "n": 4, "hi": 55, "c": 4}
    assert got["k3"] == {"name": "k3", "bp": 25, "mean": 25.0, "n": 0, "hi": None, "c": 1}      # only a padded row
    assert out.column_names == ["name", "bp", "mean", "n", "hi", "c"]


# ---------------------------------------------------------------- the C ABI
def test_the_header_s_symbol_is_the_binding_s():
    header = open(os.path.join(ROOT, "include", "giql_hip_pair_expr_agg.h")).read()
    declared = sorted(set(re.findall(r"\b(giql_hip_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))))
    assert declared == sorted(_lib.PAIR_EXPR_AGG_SYMBOLS) == ["giql_hip_pair_expr_agg_dev"]
    others = (_lib.SYMBOLS + _lib.STRING_AGG_SYMBOLS + _lib.RANGE_SET_SYMBOLS + _lib.PAIR_AGG_SYMBOLS + _lib.COVERAGE_SYMBOLS)
    assert not set(_lib.PAIR_EXPR_AGG_SYMBOLS) & set(others)
    assert "no per-pair value array" in re.sub(r"[\s*]+", " ", header).lower()     # the workspace statement
    main = open(os.path.join(ROOT, "include", "giql_hip.h")).read()
    assert "#define GIQL_HIP_ABI_VERSION 4 " in main and "pair_expr_agg" not in main
    L = _lib.load()
    assert all(hasattr(L, name) for name in _lib.PAIR_EXPR_AGG_SYMBOLS) and L.giql_hip_abi_version() == 4
    assert len(L.giql_hip_pair_expr_agg_dev.argtypes) == 12
    assert L.giql_hip_pair_expr_agg_dev(None, None, None, 0, 0, 0, None, 0, None, 0, None, None) == _lib.GIQL_ERR_INVALID
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "_lib.PAIR_EXPR_AGG_SYMBOLS" in entry


def test_struct_layout_matches_the_header(tmp_path):
    """The ctypes mirror against the real C layout: a probe compiled from the header prints sizeof / offsetof."""
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    fields = ["func", "type", "data", "valid", "first", "count", "out", "out_nn"]
    header = os.path.join(ROOT, "include", "giql_hip_pair_expr_agg.h")
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{header}"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(giql_pair_expr_agg));']
    lines += [f'  printf("{f} %zu\\n", offsetof(giql_pair_expr_agg, {f}));' for f in fields]
    lines += ['  printf("nodes %d\\n", GIQL_PAIR_EXPR_AGG_MAX_NODES);', "  return 0;", "}"]
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines))
    subprocess.run([gcc, "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert ctypes.sizeof(_lib.CPairExprAgg) == int(got["size"]) and int(got["nodes"]) == 256
    assert [f for f, _t in _lib.CPairExprAgg._fields_] == fields
    for f in fields:
        assert getattr(_lib.CPairExprAgg, f).offset == int(got[f]), f


def test_the_kernel_shares_the_reduce_function_and_adds_no_atomics_or_lds():
    csrc = os.path.join(ROOT, "giql_amd", "csrc")
    strip = lambda text: re.sub(r"//[^\n]*", "", text)   # noqa: E731
    new, old = (strip(open(os.path.join(csrc, f)).read()) for f in ("pair_expr_agg_kernels.hip.h", "merge_agg_kernels.hip.h"))
    assert "atomic" not in new and new.count("__global__") == 1 and "sel_eval_prog(" in new
    assert new.count("magg_reduce(") == 1 and old.count("magg_reduce(") == 2     # one definition, one call in each kernel
    assert "__shfl_up" not in new                                               # the scan is not copied
    assert re.findall(r"__shared__\s+(\w+)\s+(\w+)", new) == re.findall(r"__shared__\s+(\w+)\s+(\w+)", old)
    host = open(os.path.join(csrc, "giql_hip.hip")).read()
    body = host[host.index("static int pair_agg_impl("):host.index("int giql_hip_pair_agg_dev(giql_hip_ctx")]
    at = [body.index(stage) for stage in ("begin_call(", "convert_aggs(", "hipMemsetAsync(", "k_pagg_load", "run_sort(",
                                          "k_pagg_heads", "run_scan<u32>", "run_magg(", "k_pagg_scatter")]
    assert at == sorted(at)                     # in this order: the programs are checked before anything is written
    # the two stages MERGE shares with it: the conversion checks the programs, the reduction
    # launches the tiles -- this kernel or MERGE's -- and then the fold
    convert = host[host.index("static int convert_aggs("):host.index("static const giql_pair_expr_agg* column_sources(")]
    reduce_ = host[host.index("static void run_magg("):host.index("// ---------------------------------------------------------- CLUSTER / MERGE")]
    assert "check_program(" in convert and "hipMemsetAsync(" not in convert and "hipLaunchKernelGGL" not in convert
    at = [reduce_.index(k) for k in ("k_pxagg_tiles", "k_magg_tiles", "k_magg_fold")]
    assert at == sorted(at)
