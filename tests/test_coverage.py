"""Coverage depth per DISJOIN segment (``disjoin_aggregates=True``), the CPU half: the two references of
tests/_coverage_ref.py against each other, against DISJOIN's sqlite-minted pieces grouped by (chrom, start, end) and
against tests/golden/coverage.json; what the flag lowers, what it declines and what it leaves alone; the string form;
the wide-genome combine; the C ABI's declaration.  The GPU half is tests/test_coverage_gpu.py."""
import json
import os
import re
from dataclasses import replace

import numpy as np
import pytest

import _coverage_queries as Q
import _coverage_ref as R
import _disjoin_ref as D
from giql_amd import _lib
from giql_amd.plan import DISJOIN_COLUMNS, JoinPlan, PlanSide, Projection
from giql_amd.shape import ColRef, DisjoinShape, HipDeclined, SelItem, TableRef, lower_disjoin_shape
from giql_amd.table import build_tables
from giql_amd.transpile import build_plan, transpile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
RECORDED = json.load(open(os.path.join(HERE, "golden", "coverage_plans.json")))["cases"]


def as_array(rows):
    return np.array(rows, np.int64).reshape(-1, 4)


# ---------------------------------------------------------------- the references
@pytest.mark.parametrize("block", range(6))
def test_the_two_references_agree_on_small_seeded_tables(block):
    shapes = set()
    for seed in range(50 * block, 50 * block + 50):
        c, s, e, _n_chrom = R.seeded_table(seed)
        rows = list(zip(c.tolist(), s.tolist(), e.tolist()))
        for runs in (False, True):
            got = R.sweep_arrays(c, s, e, runs=runs)
            assert np.array_equal(as_array(R.sweep(rows, runs=runs)), got), (seed, runs)
        seg, run = R.sweep_arrays(c, s, e), R.sweep_arrays(c, s, e, runs=True)
        shapes |= {"merged"} if len(run) < len(seg) else set()
        shapes |= {"deep"} if len(seg) and seg[:, 3].max() >= 4 else set()
        shapes |= {"points"} if (s == e).any() else set()
        shapes |= {"duplicates"} if len({*rows}) < len(rows) else set()
        shapes |= {"chromosomes"} if len(set(c.tolist())) > 1 else set()
    assert shapes == {"merged", "deep", "points", "duplicates", "chromosomes"}


@pytest.mark.parametrize("kind", R.SHAPES)
def test_the_constructed_tables_have_the_shape_they_are_named_for(kind):
    assert [len(x) for x in R.shaped_table(kind, 0)] == [0, 0, 0]
    for n in (1, 2, 3, 127, 128, 129, 2049, 20_001):
        c, s, e = R.shaped_table(kind, n)
        assert len(c) == len(s) == len(e) == n and (s <= e).all() and (s >= 0).all()
        seg, run = R.sweep_arrays(c, s, e), R.sweep_arrays(c, s, e, runs=True)
        if kind == "distinct":
            assert len(seg) == 2 * n - 1 and len(np.unique(np.concatenate([s, e]))) == 2 * n
        elif kind == "identical":
            assert seg.tolist() == [[0, 7, 19, n]]
        elif kind == "chain":
            assert len(seg) == n and (seg[:, 3] == 1).all() and run.tolist() == [[0, 0, 10 * n, 1]]
        elif kind == "alternating":
            assert len(run) == len(seg) and (n < 3 or set(seg[:, 3].tolist()) >= {1, 2})
            assert (seg[1:, 1] == seg[:-1, 2]).all()                      # abutting throughout: only the depth separates
        elif kind == "nested":
            assert len(seg) == 2 * n - 1 and seg[:, 3].max() == n and seg[0, 3] == seg[-1, 3] == 1
        elif kind == "points":
            assert len(seg) == 0 and len(run) == 0
        elif kind == "points-inside":
            assert len(run) == max(n // 3, 1) and (n < 6 or len(seg) > len(run)) and (seg[:, 3] == 1).all()


SELF_CASES = [c for c in D.golden_cases() if c["reference"] is None]


def test_disjoin_goldens_hold_39_self_mode_cases():
    assert len(SELF_CASES) == 39 and sum(len(c["expected"]) for c in SELF_CASES) == 501


@pytest.mark.parametrize("case", SELF_CASES, ids=lambda c: c["id"])
def test_references_equal_disjoin_pieces_grouped_by_segment(case):
    """The recipe's GROUP BY over DISJOIN's sqlite-minted pieces: exactly the segments and counts of both references."""
    names = sorted({r[0] for r in case["target"]})
    rows = [(names.index(r[0]), r[1], r[2]) for r in case["target"]]
    want = R.group_pieces([r[0] for r in rows], case["expected"])
    assert R.sweep(rows, case["encoding"]) == want
    cols = [np.array(x, np.int64) for x in zip(*rows)]
    assert np.array_equal(R.sweep_arrays(*cols, case["encoding"]), as_array(want))
    assert np.array_equal(R.sweep_arrays(*cols, case["encoding"], runs=True), as_array(R.sweep(rows, case["encoding"], runs=True)))


def test_the_disjoin_goldens_hold_abutting_segments_of_equal_depth():
    """10 pairs in the half-open cases, where raw coordinates abut as the SQL recipe sees them; the closed cases add
    11 that abut on the canonical axis only (the kernel's run form merges those too)."""
    merged = {"half_open": 0, "closed": 0}
    for case in SELF_CASES:
        names = sorted({r[0] for r in case["target"]})
        rows = [(names.index(r[0]), r[1], r[2]) for r in case["target"]]
        merged[case["encoding"][1]] += len(R.sweep(rows, case["encoding"])) - len(R.sweep(rows, case["encoding"], runs=True))
    assert merged == {"half_open": 10, "closed": 11}


def golden_ids(case):
    names = sorted({r[0] for r in case["rows"]})
    ids = lambda rows: [[names.index(r[0])] + list(r[1:]) for r in rows]  # noqa: E731
    return names, ids(case["rows"]), ids(case["segments"]), None if case["runs"] is None else ids(case["runs"])


def test_coverage_goldens_cover_the_four_encodings():
    cases = R.golden_cases()
    assert len(cases) == 60 and {tuple(c["encoding"]) for c in cases} == set(D.OFFSETS)
    assert all((c["runs"] is None) == (c["encoding"][1] == "closed") for c in cases)
    assert sum(len(c["segments"]) - len(c["runs"]) for c in cases if c["runs"] is not None) >= 20
    assert os.path.getsize(R.GOLDEN) < 256 * 1024


@pytest.mark.parametrize("case", R.golden_cases(), ids=lambda c: c["id"])
def test_references_equal_the_sqlite_minted_coverage(case):
    _names, rows, segments, runs = golden_ids(case)
    cols = [np.array(x, np.int64) for x in zip(*rows)]
    assert R.sweep(rows, case["encoding"]) == segments
    assert np.array_equal(R.sweep_arrays(*cols, case["encoding"]), as_array(segments))
    if runs is not None:
        assert R.sweep(rows, case["encoding"], runs=True) == runs
        assert np.array_equal(R.sweep_arrays(*cols, case["encoding"], runs=True), as_array(runs))


# ---------------------------------------------------------------- plans
@pytest.mark.parametrize("name", sorted(Q.ACCEPTED))
def test_accepted_forms_lower_with_the_flag(name):
    query, segments = Q.ACCEPTED[name]
    plan = build_plan(query, Q.TABLES, disjoin_aggregates=True)
    assert plan.kind == "DISJOIN" and plan.segments == segments and plan.right is None
    assert JoinPlan.from_string(plan.to_string()) == plan and JoinPlan.from_dict(plan.to_dict()) == plan
    assert '"segments":"%s"' % segments in plan.to_string()
    assert transpile(query, Q.TABLES, dialect="hip", disjoin_aggregates=True) == plan.to_string()
    counts = [p for p in plan.projection if p.side == "count"]
    assert all(p.side in ("disjoin", "count") for p in plan.projection)
    assert bool(counts) == (segments == "depth") or name == "depth_count_only"
    if segments == "runs":
        assert [p.name for p in plan.projection] == ["chrom", "start", "end"]
        assert [p.column for p in plan.projection] == list(DISJOIN_COLUMNS)
    if segments == "distinct":   # the plan of the parent commit, marked
        assert replace(plan, segments=None).to_string() == RECORDED[f"accepted/{name}"]["plan"]


def test_accepted_forms_in_detail():
    plan = build_plan(Q.ACCEPTED["depth_order_limit"][0], Q.TABLES, disjoin_aggregates=True)
    assert plan.order_by == (("depth", True, False), ("chrom", False, True), ("start", False, True))
    assert (plan.limit, plan.offset) == (3, 1)
    assert plan.projection[-1] == Projection("count", "*", "depth")
    plan = build_plan(Q.ACCEPTED["depth_order_hidden_key"][0], Q.TABLES, disjoin_aggregates=True)
    assert plan.projection[-1] == Projection("disjoin", "disjoin_end", "__giql_o0") and plan.order_by[0][0] == "__giql_o0"
    plan = build_plan(Q.ACCEPTED["depth_two_counts"][0], Q.TABLES, disjoin_aggregates=True)
    assert [p.name for p in plan.projection] == ["a", "disjoin_chrom", "disjoin_start", "disjoin_end", "b"]
    plan = build_plan(Q.ACCEPTED["depth_closed_target"][0], Q.TABLES, disjoin_aggregates=True)
    assert plan.left.encoding == ("1based", "closed")
    plan = build_plan(Q.ACCEPTED["runs_order_limit"][0], Q.TABLES, disjoin_aggregates=True)
    assert plan.order_by == (("chrom", True, False), ("start", False, True)) and plan.limit == 4
    assert build_plan(Q.ACCEPTED["runs_one_based_half_open"][0], Q.TABLES, disjoin_aggregates=True).left.encoding == \
        ("1based", "half_open")


@pytest.mark.parametrize("name", sorted(Q.DECLINED))
def test_declines_name_their_reason(name):
    query, reason = Q.DECLINED[name]
    with pytest.raises(HipDeclined) as exc:
        build_plan(query, Q.TABLES, disjoin_aggregates=True)
    assert reason in str(exc.value)


def test_every_decline_has_a_reason_of_its_own():
    groups = {}
    for name, (query, reason) in Q.DECLINED.items():
        groups.setdefault(reason, []).append(name)
    for need in ("COUNT(*) without an alias", "COUNT(name)", "SUM(", "target column 'name'", "other than exactly",
                 "reference :=", "WHERE over the rows of DISJOIN", "HAVING over the rows of DISJOIN", "MERGE distance",
                 "stranded", "predicate other than", "aggregate beside MERGE", "other than the coverage",
                 "closed-interval target"):
        assert need in groups


def test_the_closed_target_decline_of_the_run_recipe_says_why():
    for table in ("closed1", "closed0"):
        with pytest.raises(HipDeclined, match=r"closed-interval target.*never touch"):
            build_plan(Q.RUNS.replace("features", table), Q.TABLES, disjoin_aggregates=True)
        assert build_plan(Q.DEPTH.replace("features", table), Q.TABLES, disjoin_aggregates=True).segments == "depth"


@pytest.mark.parametrize("name", sorted(Q.all_queries()))
def test_without_the_flag_every_query_lowers_as_recorded(name):
    query = Q.all_queries()[name]
    assert Q.outcome(build_plan, query) == RECORDED[name]
    assert Q.outcome(build_plan, query, disjoin_aggregates=False) == RECORDED[name]
    if name.startswith("outside/"):
        assert Q.outcome(build_plan, query, disjoin_aggregates=True) == RECORDED[name]


def test_the_recording_names_the_parent_commit_and_every_query():
    doc = json.load(open(os.path.join(HERE, "golden", "coverage_plans.json")))
    assert re.fullmatch(r"[0-9a-f]{40}", doc["recorded_at_commit"]) and set(doc["cases"]) == set(Q.all_queries())
    declines = [v["message"] for k, v in doc["cases"].items() if "error" in v]
    assert any(m.startswith("GROUP BY / aggregates over the rows of DISJOIN") for m in declines)
    assert any(m.startswith("CLUSTER / MERGE over a sub-query") for m in declines)


def test_the_segments_field_is_absent_unless_set_and_is_checked():
    left = PlanSide("features", "features")
    plain = JoinPlan("DISJOIN", left, None, (Projection("star", "*", "*"),))
    assert "segments" not in plain.to_dict() and "segments" not in plain.to_string()
    assert JoinPlan.from_string(plain.to_string()).segments is None
    for form in ("distinct", "depth", "runs"):
        marked = replace(plain, segments=form)
        assert marked.to_dict()["segments"] == form and JoinPlan.from_string(marked.to_string()) == marked
    with pytest.raises(ValueError, match="segments"):
        replace(plain, segments="histogram")
    with pytest.raises(ValueError, match="segments"):
        JoinPlan("DISJOIN", left, PlanSide("other", "other"), (Projection("star", "*", "*"),), segments="depth")
    with pytest.raises(ValueError, match="segments"):
        JoinPlan("MERGE", left, None, (), segments="runs")


def test_the_shared_gate_keeps_declining_without_the_flag_or_the_column_list():
    """The plugin calls ``lower_disjoin_shape(shape, tables)``: no flag, no GROUP BY column list."""
    tables = build_tables(Q.TABLES)
    keys = [ColRef(None, False, c) for c in DISJOIN_COLUMNS]
    items = [SelItem(k) for k in keys] + [SelItem(None, "depth", "COUNT")]

    def shape(**kw):
        return DisjoinShape(items=list(items), target=TableRef("features", "features"), group_by=True, **kw)

    for kw, flag in (({}, False), ({}, True), ({"group_cols": list(keys)}, False)):
        with pytest.raises(HipDeclined, match="GROUP BY / aggregates over the rows of DISJOIN"):
            lower_disjoin_shape(shape(**kw), tables, **({"disjoin_aggregates": True} if flag else {}))
    assert lower_disjoin_shape(shape(group_cols=list(keys)), tables, disjoin_aggregates=True).segments == "depth"


# ---------------------------------------------------------------- the wide-genome combine
def test_wide_merge_combines_segments_of_two_groups():
    torch = pytest.importorskip("torch")
    from giql_amd import wide

    c = np.array([2, 0, 1, 0, 2, 1, 0], np.int64)
    s = np.array([5, 0, 7, 4, 5, 0, 8], np.int64)
    e = np.array([9, 6, 9, 8, 12, 3, 8], np.int64)
    for runs in (False, True):
        parts = []
        for group in ([0, 2], [1]):
            rows = np.nonzero(np.isin(c, group))[0]
            got = R.sweep_arrays(c[rows], s[rows], e[rows], runs=runs)
            parts.append((torch.from_numpy(rows), None, tuple(
                torch.from_numpy(np.ascontiguousarray(got[:, k])).to(torch.int64 if k == 3 else torch.int32) for k in range(4))))
        out = wide.merge(parts, torch.device("cpu"))
        assert [t.dtype for t in out] == [torch.int32, torch.int32, torch.int32, torch.int64]
        assert np.array_equal(np.stack([t.numpy().astype(np.int64) for t in out], 1), R.sweep_arrays(c, s, e, runs=runs))
    empty = wide.merge([], torch.device("cpu"))
    assert [int(t.numel()) for t in empty] == [0, 0, 0, 0]


# ---------------------------------------------------------------- the C ABI
def test_the_entry_point_lives_in_an_extension_header_of_its_own():
    header = open(os.path.join(ROOT, "include", "giql_hip_coverage.h")).read()
    declared = re.findall(r"\b(giql_hip_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert declared == _lib.COVERAGE_SYMBOLS == ["giql_hip_coverage_dev"]
    assert re.search(r"#define\s+GIQL_COV_RUNS\s+1u", header) and _lib.COV_RUNS == 1
    main = open(os.path.join(ROOT, "include", "giql_hip.h")).read()
    assert "giql_hip_coverage" not in main and "GIQL_COV" not in main and re.search(r"#define\s+GIQL_HIP_ABI_VERSION\s+4\b", main)
    assert not set(_lib.COVERAGE_SYMBOLS) & set(_lib.SYMBOLS + _lib.RANGE_SET_SYMBOLS + _lib.STRING_AGG_SYMBOLS
                                                + _lib.PAIR_AGG_SYMBOLS)


def test_the_kernels_reuse_disjoins_stages_and_need_no_atomics():
    host = open(os.path.join(ROOT, "giql_amd", "csrc", "giql_hip.hip")).read()
    body = host[host.index("static int giql_hip_coverage_dev_impl"):host.index("int giql_hip_coverage_dev(giql_hip_ctx")]
    for stage in ("begin_call(", "run_events(", "k_cov_depth", "k_cov_run_heads", "k_cov_fill"):
        assert stage in body, stage
    # DISJOIN's front is one stage that DISJOIN's plan calls as well
    sweep = host[host.index("static int run_events("):host.index("static int finish_events(")]
    for stage in ("run_spans(", "k_dj_events", "k_digit_offsets", "run_sort_onesweep(ctx, st, E.sb, sort_by_start(", "k_dj_flags"):
        assert stage in sweep, stage
    assert "run_events(" in host[host.index("static int giql_hip_disjoin_plan_dev_impl"):host.index("int giql_hip_disjoin_plan_dev(giql_hip_ctx")]
    assert sweep.count("run_scan<u32>") == 2 and body.count("run_scan<u32>") == 1
    assert "with_order_fallback" in host[host.index("int giql_hip_coverage_dev(giql_hip_ctx"):][:600]
    for gone in ("k_dj_count", "k_dj_fill", "k_dj_covered", "lo_first"):
        assert gone not in body
    kernels = open(os.path.join(ROOT, "giql_amd", "csrc", "coverage_kernels.hip.h")).read()
    code = re.sub(r"//[^\n]*", "", kernels)
    assert "atomic" not in code and "__global__" in code
