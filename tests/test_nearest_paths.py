"""NEAREST (k = 1 and its 32-bit form), NEAREST k > 1 and group_rows on every path of their kernels, under every form of
their sorts and on both tie plans -- needs a GPU (but for the check of the cases themselves).

The family alone needs B in (start, end) order: from one sort by start plus ``k_fix_start_ties`` (runs of at most
NEAREST_TIE_MAX = 32 equal keys ordered in place), or -- for good on a context that met a longer run
(``guess.nearest_two_sorts``) -- from ``run_sort_two_keys``; NEAREST k adds the (end, start) view with its own tie pass, or a
third stable sort.  ``k_nearest`` / ``k_nearest_k`` (``giql_amd/csrc/aux_kernels.hip.h``) then answer every block of 1,024 A
rows from LDS stages around the block's bracket of B and read whatever lies outside from global memory.

Truth is the oracle's brute force (``tests/_nearest_cases.py``, once per case); everything is integer and every comparison
exact: NEAREST rows as (distance, start, end) per A row and slot in order, which slots are -1, and -- B holds no duplicate
row unless a case says so -- the row ids themselves; ``group_of_row`` equals the inverse of ``np.unique`` over (chrom, start,
end).  One truth for every form and plan: their answers are identical to each other because each is identical to it.

Which path ran.  The tie plan is read from ``stats()["phase_launches"]["aux"]`` (``AUX`` below, held to the recorded
launches of ``tests/golden/row_op_launches.json`` by the CPU check): the one-sort plan launches ``k_fix_start_ties`` there,
the two-sort plan does not.  ``linearize`` tells a NEAREST call that built its keys from the raw columns (2 launches) from
the layout probe and the ordinary call (4).  Whether a block is served from its LDS stage has no statistic:
``test_cases_are_what_they_claim`` proves the bracket widths on the CPU, for A fully sorted and for A ordered by
``key >> 8`` / ``key >> 16`` with ties in input order (what ``row_skip`` may leave), under both key layouts.

The sort forms are the ``FORMS`` of ``tests/test_disjoin_paths.py``: one context per form runs the cases once on the
one-sort plan, meets the pile-up table, and runs them again on the two-sort plan it keeps.
"""
import json
import os

import numpy as np
import pytest

import _nearest_cases as N
from _nearest_cases import NR_BACK, NR_CAP, NR_CHROMS, NR_TQ, NRK_CAP, NRK_EBACK, TIE_MAX
from test_disjoin_paths import FORMS, OS_TILE, _assert_form, _engine

torch = pytest.importorskip("torch")

gpu = pytest.mark.gpu        # (the cases are checked without one: test_cases_are_what_they_claim)

DEV = "cuda:0"
CASES = N.cases()
# phase_launches["aux"] of a call: (one-sort plan, two-sort plan) -- run_pmax launches three, k_fix_start_ties once per view
AUX = {"nearest": (4, 3), "nearest32": (4, 3), "nearest_k": (5, 3), "group_rows": (1, 0)}
LINEARIZE = {"keys-from-raw-columns": 2, "linearized": 4}
SETTINGS = ((False, None), (True, None), (False, "md"), (True, "md"))     # (signed, max_distance: the case's small one)
FORM_KS = (3, 16)
FORM_CASES = ["blocks-1025", "bracket-wider-than-both", "end-runs-2-31-32", "chromosome-clamps"] + \
             [c for c in CASES if c.startswith("sort/")]


# ---------------------------------------------------------------- the cases, on the CPU
def test_the_launch_counts_are_the_recorded_ones():
    with open(os.path.join(N.HERE, "golden", "row_op_launches.json")) as f:
        rec = {k: v["phase_launches"] for k, v in json.load(f)["cases"].items()}
    assert (rec["nearest/first"]["aux"], rec["nearest/pile/second"]["aux"]) == AUX["nearest"]
    assert (rec["nearest32"]["aux"], rec["nearest/pile/first"]["aux"]) == AUX["nearest32"]
    for k in ("k3", "k16"):
        assert (rec[f"nearest-{k}/one-sort"]["aux"], rec[f"nearest-{k}/two-sorts"]["aux"]) == AUX["nearest_k"]
    assert (rec["group-rows/one-sort"]["aux"], rec["group-rows/two-sorts"].get("aux", 0)) == AUX["group_rows"]
    assert rec["group-rows/pile/first"].get("aux", 0) == 0          # the repeat's launches are the call's
    assert rec["nearest/first"]["linearize"] == rec["nearest/pile/second"]["linearize"] == LINEARIZE["linearized"]
    assert rec["nearest/second"]["linearize"] == rec["nearest32"]["linearize"] == LINEARIZE["keys-from-raw-columns"]


def test_cases_are_what_they_claim():
    got = N.header_constants()
    for name, value in N.CONSTANTS.items():
        assert got[name] == value, (name, got[name], "rebuild the cases of tests/_nearest_cases.py around it")
    assert got["NR_NT"] * got["GIQL_NR_ITEMS"] == NR_TQ
    assert 2 * NRK_CAP == NR_CAP         # (so no bracket is 2 x NRK_CAP wide and NR_CAP / 2 at most: see case 2)
    for case in CASES.values():
        assert case.a.n <= 3_100 and (case.b.n <= 12_300 or case.id.startswith("sort/")), case.id
        assert case.has_dups() == case.dups, case.id
        assert (case.a.end >= case.a.start).all() and (case.b.end >= case.b.start).all(), case.id
        starts, ends = case.longest_runs()
        want = {"one-sort": starts <= TIE_MAX and ends <= TIE_MAX, "k-flags": starts <= TIE_MAX < ends, "all-flag": starts > TIE_MAX}
        assert want[case.plan], (case.id, case.plan, starts, ends)
        if case.n_chrom == 1:            # key == start in both layouts
            assert min(case.a.start.min(), case.b.start.min()) == 0 and case.aligned(), case.id
            assert all(np.array_equal(k, c) for lay in (False, True) for k, c in
                       zip(case.keys(lay), (case.a.start, case.a.end, case.b.start, case.b.end))), case.id
        # On a linear axis an end key never reaches the next chromosome's first key, so lower_bound(B starts, a.end) lies
        # inside the row's chromosome by itself: the kernels' `hi < blo` / `hi > bhi` clamps bound nothing here (no table can
        # tell them from their absence); what keeps a walk on its chromosome is `dn < bhi` and `run_lo == elo` (case 9).
        for lay in case.layouts():
            _ak, ae, bk, _be = case.keys(lay)
            chrom_sorted = case.b.chrom[np.argsort(bk, kind="stable")]
            assert np.all(np.diff(chrom_sorted) >= 0), case.id
            hi = np.searchsorted(np.sort(bk), ae, "left")
            assert np.all(np.searchsorted(chrom_sorted, case.a.chrom, "left") <= hi), case.id
            assert np.all(hi <= np.searchsorted(chrom_sorted, case.a.chrom, "right")), case.id
    order = list(CASES)
    assert [CASES[c].plan for c in order] == sorted((CASES[c].plan for c in order), key=["one-sort", "k-flags", "all-flag"].index)
    assert set(FORM_CASES) <= set(CASES) and order.index(N.PILE_UP) == len(order) - 1

    # 1: block edges -- every bracket (plus NR_BACK below, k = 17 above) fits the smaller stage
    for n in N.BLOCK_SIZES:
        case = CASES[f"blocks-{n}"]
        blocks = case.blocks(k=17)
        assert case.a.n == n and case.b.n == 3000 and case.n_chrom == 3 and len(blocks) == 3 * len(case.layouts()) * -(-n // NR_TQ)
        assert all(b["staged"] and b["staged_k"] and b["staged_e"] for b in blocks), case.id
    assert max(b["width"] for b in CASES["blocks-2049"].blocks()) > 600
    # 4: ... and k = 2,100 carries the stage past NRK_CAP in the full block, whatever its order
    case = CASES["blocks-1025"]
    assert set(case.ks) == {2, 15, 16, 17, 2100}
    assert all(b["staged_k"] for b in case.blocks(k=17)) and not any(b["staged_k"] for b in case.blocks(k=2100) if b["full"])
    # 2: staged by k_nearest, not by k_nearest_k (k = 2): as far from both caps as 2 * NRK_CAP = NR_CAP allows
    case = CASES["bracket-between-the-caps"]
    full = [b for b in case.blocks(k=2) if b["full"]]
    assert len(full) == 2 * 3 * 2 and all(b["staged"] and not b["staged_k"] for b in full)
    assert all(NRK_CAP * 5 // 4 <= b["width"] and b["width"] + NR_BACK + 1 <= NR_CAP * 4 // 5 for b in full), [b["width"] for b in full]
    # 3: wider than both, twice over; the rest block stages
    case = CASES["bracket-wider-than-both"]
    blocks = case.blocks(k=2)
    assert all(b["width"] >= 2 * NR_CAP and not b["staged"] and not b["staged_k"] for b in blocks if b["full"])
    assert all(b["staged"] and b["staged_k"] and b["width"] > 100 for b in blocks if not b["full"]) and case.b.n <= 12_000
    # 5: the plateau of the prefix maximum starts at row 0, more than NR_BACK rows below every bracket; 300 > NRK_EBACK
    case = CASES["gallop-below-the-stage"]
    by_start = np.lexsort((case.b.end, case.b.start))
    pmax = np.maximum.accumulate(case.b.end[by_start])
    assert by_start[0] == 0 and case.b.end[0] == case.b.end.max() and np.all(pmax == pmax[-1]) and case.b.n == 601
    assert case.a.start.min() >= case.b.end.max() and 300 in case.ks and 300 > NRK_EBACK
    for b in case.blocks(k=2):
        assert b["w_lo"] == b["w_hi"] == case.b.n and b["w_lo"] - NR_BACK > 0 and b["staged"] and b["staged_k"]
        assert b["e_hi"] == case.b.n and b["staged_e"] and b["e0"] > case.b.n - 300
    # 6 / 7: runs of equal ends with distinct starts; the long one lies across e0 of the second block's stage
    for cid, long_run in (("end-runs-2-31-32", 32), ("end-run-33", 33)):
        case = CASES[cid]
        e_sorted = np.sort(case.b.end)
        ends, first, count = np.unique(e_sorted, return_index=True, return_counts=True)
        assert {2, 31, long_run} <= set(count.tolist()) and count.max() == long_run and (count > 1).sum() > 40, cid
        assert len(np.unique(case.b.start)) > case.b.n - 200 and case.longest_runs()[0] <= 8
        second = [b for b in case.blocks(k=224) if not b["first"]]
        assert len(second) == 3 * 2 and all(b["staged_e"] and b["staged_k"] for b in case.blocks(k=224))
        for b in second:
            lo = int(first[count == long_run][0])
            assert b["e_lo"] == case.b.n and lo < b["e0"] < lo + long_run - 1, (cid, lo, b["e0"])
            assert b["e_lo"] - 224 < lo                                       # k = 224 walks past its head
        in_order = case.b.start[np.argsort(case.b.end, kind="stable")]       # the runs arrive out of start order
        assert any(np.any(np.diff(in_order[f:f + c]) < 0) for f, c in zip(first, count) if c > 1)
        assert (case.a.start == N.S_BLOCK1).sum() >= 12 and case.b.end.max() < N.S_BLOCK1
    assert 224 in CASES["end-runs-2-31-32"].ks
    # 8: runs of equal starts with distinct ends, probed by rows inside their ends; duplicates inside a 32-run
    for cid, long_run in (("start-run-32", 32), ("start-run-33", 33), ("start-run-32-with-equal-rows", 32)):
        case = CASES[cid]
        starts, count = np.unique(case.b.start, return_counts=True)
        assert count.max() == long_run and starts[count.argmax()] == N.RUN_START and 31 in count.tolist(), cid
        run = case.b.end[case.b.start == N.RUN_START]
        assert np.any(np.diff(run) < 0) and case.longest_runs()[1] <= 8
        inside = (case.a.start > N.RUN_START) & (case.a.start < run.max())
        assert inside.sum() >= 10 and (case.a.end == N.RUN_START).sum() >= 1
        if case.dups:
            ends, per_end = np.unique(run, return_counts=True)
            assert sorted(per_end[per_end > 1].tolist()) == [3, 5] and case.groups()[1] == case.b.n - 6
        else:
            assert len(np.unique(run)) == long_run
    # 9: one block over five chromosomes; who has rows where; linear neighbours on another chromosome are nearer
    case = CASES["chromosome-clamps"]
    a, b = case.a, case.b
    assert case.n_chrom == 5 and a.n <= NR_TQ and len(case.blocks()) == 3 * 2 and 4 in case.ks
    assert not (b.chrom == 2).any() and not (a.chrom == 0).any() and (a.chrom == 2).sum() > 100 and (b.chrom == 0).sum() > 50
    assert a.end[a.chrom == 1].max() < b.start[b.chrom == 1].min() and a.start[a.chrom == 3].min() > b.end[b.chrom == 3].max()
    assert (b.chrom == 4).sum() == 2 and (a.chrom == 4).sum() > 100
    for lay in case.layouts():
        ak, ae, bk, be = case.keys(lay)
        for c in (1, 2, 3):
            for i in np.nonzero(a.chrom == c)[0]:
                gap = np.where(bk >= ae[i], bk - ae[i], np.where(be <= ak[i], ak[i] - be, 0))
                assert b.chrom[gap.argmin()] != c, (c, i)
    wi, _wd = case.nearest_k(4)
    assert (wi[a.chrom == 2] == -1).all() and ((wi[a.chrom == 4] >= 0).sum(1) == 2).all() and (wi[a.chrom == 1] >= 0).all()
    # 10: around the LDS limit of the chromosome tables
    for n in (NR_CHROMS, NR_CHROMS + 1, NR_CHROMS + 2):
        case = CASES[f"chromosomes-{n}"]
        assert case.n_chrom == n and all(len(np.unique(t.chrom)) == n and np.bincount(t.chrom).max() <= 8 for t in (case.a, case.b))
    # 11: the rows written by hand are the oracle's, the C brute force's and the row-by-row Python's
    case = CASES["distance-edges"]
    for (k, signed, md), want in case.hand.items():
        assert N.triples(*case.nearest_k(k, signed, md), case.b) == want, (k, signed, md)
        py = ora_py_nearest_k(case, k, signed, md)
        assert py == want, (k, signed, md)
        if k == 1:
            wi, wd = case.nearest(signed, md)
            assert N.triples(wi[:, None], wd[:, None], case.b) == want, (signed, md)
    # 12: the sort shapes keep what the CLUSTER / MERGE cases claim of their starts
    for n in (OS_TILE - 1, OS_TILE, OS_TILE + 1):
        assert CASES[f"sort/rows-{n}"].b.n == n
    s = CASES["sort/empty-and-one-row-buckets"].b.start
    for w in (13, 14, 15, 16):
        per = np.bincount(s >> w, minlength=(4 << 16) >> w)
        assert per[(65_536 + 5) >> w] == 1 and (per == 0).any() and per.max() > 100, w
    case = CASES["sort/both-ends-of-the-axis"]
    assert not case.aligned() and case.keys(False)[2].min() == 0 and case.keys(False)[3].max() == 2**32 - 2
    s = CASES["sort/hot-bucket-above-bs-cap"].b.start
    hot = (s >= 2 * 65_536) & (s < 2 * 65_536 + 8_192)
    assert hot.sum() >= 9_000 and np.bincount(s[~hot] >> 13).max() < 4096
    case = CASES[N.PILE_UP]
    assert case.b.n == 20_000 and len(np.unique(case.b.start)) == 200 and case.dups and case.longest_runs()[0] > TIE_MAX
    for cid in FORM_CASES:               # the small max_distance keeps some rows and drops some
        wi, _wd = CASES[cid].nearest(False, CASES[cid].md)
        assert 0 < (wi >= 0).sum() < CASES[cid].a.n, cid


def ora_py_nearest_k(case, k, signed, md):
    from oracle import pyoracle as ora

    rows = ora.py_nearest_k(case.a, case.b, k, signed=signed, max_distance=md)
    return [[(int(d), int(case.b.start[j]), int(case.b.end[j])) for j, d in row] for row in rows]


# ---------------------------------------------------------------- device side
_RESIDENT = {}


def resident(cid):
    from giql_amd.engine import DeviceSide

    if cid not in _RESIDENT:
        case = CASES[cid]
        _RESIDENT[cid] = tuple(DeviceSide.from_numpy(t.chrom, t.start, t.end, device=DEV) for t in (case.a, case.b))
    return _RESIDENT[cid]


def _context(env, form):
    e = _engine(env)
    e.form, e.two_sorts = form, False        # two_sorts: what the calls so far must have left in guess.nearest_two_sorts
    return e


def _plan_ran(e, op, case, what):
    """The call that just returned ran the plan the context's history and the table ask for."""
    if (case.flags_k if op == "nearest_k" else case.flags_1):
        e.two_sorts = True                   # (a fresh context flags, repeats on the two-sort plan and keeps it)
    aux = e.stats()["phase_launches"]["aux"]
    assert aux == AUX[op][e.two_sorts], (what, op, "two-sort plan" if e.two_sorts else "one-sort plan", aux)
    if e.form is not None and op != "group_rows":
        _assert_form(e)


def _nearest(e, case, signed, md, what, ops=("nearest", "nearest32")):
    da, db = resident(case.id)
    wi, wd = case.nearest(signed, md)
    for op in ops:
        if op == "nearest32" and np.abs(wd).max() >= 2**31:       # the 32-bit form refuses what it cannot hold
            from giql_amd import _lib

            with pytest.raises(_lib.GiqlHipError) as exc:
                e.nearest32(da, db, case.n_chrom, signed=signed, max_distance=md)
            assert exc.value.code == _lib.GIQL_ERR_INVALID, (what, op)
            continue
        if op == "nearest":
            idx, dist = (t.cpu().numpy() for t in e.nearest(da, db, case.n_chrom, signed=signed, max_distance=md))
        else:
            rec = e.nearest32(da, db, case.n_chrom, signed=signed, max_distance=md).cpu().numpy()
            idx, dist = rec[:, 0], rec[:, 1].astype(np.int64)
        _plan_ran(e, op, case, what)
        N.same_rows(case.b, idx, dist, wi, wd, not case.dups, (what, op, signed, md))
    return idx, dist


def _nearest_k(e, case, k, signed, md, what):
    da, db = resident(case.id)
    idx, dist = (t.cpu().numpy() for t in e.nearest_k(da, db, case.n_chrom, k, signed=signed, max_distance=md))
    _plan_ran(e, "nearest_k", case, what)
    N.same_rows(case.b, idx, dist, *case.nearest_k(k, signed, md), not case.dups, (what, "nearest_k", k, signed, md))
    return idx, dist


def _group_rows(e, case, what):
    _da, db = resident(case.id)
    gid, rep = e.group_rows(db, case.n_chrom)
    _plan_ran(e, "group_rows", case, what)
    want, n_groups = case.groups()
    gid_h, rep_h = gid.cpu().numpy(), rep.cpu().numpy()
    assert rep_h.shape == (n_groups,) and np.array_equal(gid_h, want), (what, "group_of_row")
    assert np.array_equal(want[rep_h], np.arange(n_groups)), (what, "rep_row")
    vals = np.random.default_rng(case.b.n).integers(-2**40, 2**40, case.b.n)
    sums = np.zeros(n_groups, np.int64)
    np.add.at(sums, want, vals)
    got = e.segment_sum(torch.from_numpy(vals).to(DEV), gid, n_groups).cpu().numpy()
    assert np.array_equal(got, sums), (what, "segment_sum")


# ---------------------------------------------------------------- the default form: every case, every operator
@pytest.fixture(scope="module")
def eng():
    e = _context({}, None)
    yield e
    e.close()


@gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_every_case_on_the_default_form(eng, cid):
    case = CASES[cid]
    for signed, md in SETTINGS:
        md = case.md if md else None
        _nearest(eng, case, signed, md, cid)
    for k in case.ks:
        _nearest_k(eng, case, k, k % 2 == 1, None, cid)
    _nearest_k(eng, case, 2, True, case.md, cid)
    _nearest_k(eng, case, 16, False, case.md, cid)
    if cid == "sort/both-ends-of-the-axis":
        assert eng.stats()["span"] == 2**32 - 1
    _group_rows(eng, case, cid)
    if case.hand:
        da, db = resident(cid)
        for (k, signed, md), want in case.hand.items():
            idx, dist = (t.cpu().numpy() for t in eng.nearest_k(da, db, case.n_chrom, k, signed=signed, max_distance=md))
            assert N.triples(idx, dist, case.b) == want, ("nearest_k", k, signed, md)
            if k == 1:
                idx, dist = (t.cpu().numpy() for t in eng.nearest(da, db, case.n_chrom, signed=signed, max_distance=md))
                assert N.triples(idx[:, None], dist[:, None], case.b) == want, ("nearest", signed, md)
                rec = eng.nearest32(da, db, case.n_chrom, signed=signed, max_distance=md).cpu().numpy()
                assert N.triples(rec[:, :1], rec[:, 1:], case.b) == want, ("nearest32", signed, md)


@gpu
def test_three_calls_in_a_row_probe_raw_column_keys_and_the_missed_layout():
    """NEAREST k = 1 three times on every table, on one fresh context: its first call probes the aligned layout, the
    calls after it build their keys from the raw columns while the layout holds.  ``both-ends-of-the-axis`` (two
    chromosomes of 2^31 positions: 256 buckets of 2^24) is the table for which it does not: that call misses its guess,
    repeats linearized, and the context builds no keys from raw columns again.  The three results are equal."""
    e = _context({}, None)
    aligned = -1
    seen = set()
    try:
        for cid, case in CASES.items():
            for rep in range(3):
                hist_ok = not e.two_sorts and case.n_chrom <= N.MM_HIST_CHROMS
                keygen, probe = hist_ok and aligned == 1, hist_ok and aligned == -1
                idx, dist = _nearest(e, case, rep == 1, None, (cid, "call", rep), ops=("nearest",))
                if keygen or probe:
                    aligned = int(case.aligned())
                path = "keys-from-raw-columns" if keygen and case.aligned() and not case.flags_1 else "linearized"
                seen.add(("probe" if probe else "missed" if keygen and not case.aligned() else path))
                assert e.stats()["phase_launches"]["linearize"] == LINEARIZE[path], (cid, rep, path)
                first = (idx, dist) if rep == 0 else first          # (the second call is signed)
                assert np.array_equal(idx, first[0]) and np.array_equal(np.abs(dist), first[1]), (cid, rep)
    finally:
        e.close()
    assert seen == {"probe", "keys-from-raw-columns", "missed", "linearized"}


# ---------------------------------------------------------------- fresh contexts: who leaves the one-sort plan
def _fresh_call(cid, op):
    e = _context({}, None)
    try:
        case = CASES[cid]
        for _ in range(2):                   # the second call starts on the plan the first one left
            if op == "nearest":
                _nearest(e, case, True, None, (cid, "fresh"))
            elif op == "nearest_k":
                _nearest_k(e, case, 3, True, None, (cid, "fresh"))
                _nearest_k(e, case, 16, False, None, (cid, "fresh"))
            else:
                _group_rows(e, case, (cid, "fresh"))
        return e.two_sorts
    finally:
        e.close()


@gpu
@pytest.mark.parametrize("op", ["nearest", "nearest_k", "group_rows"])
@pytest.mark.parametrize("cid,leaves", [
    ("end-runs-2-31-32", ()), ("start-run-32", ()), ("start-run-32-with-equal-rows", ()),
    ("end-run-33", ("nearest_k",)), ("start-run-33", ("nearest", "nearest_k", "group_rows"))])
def test_runs_of_32_stay_on_the_one_sort_plan_and_runs_of_33_leave_it(cid, leaves, op):
    """A fresh context each: ``_plan_ran`` holds every call to the plan the table asks for -- 33 equal ends flag through
    the (end, start) view's tie pass, which NEAREST k alone runs."""
    assert _fresh_call(cid, op) == (op in leaves)


# ---------------------------------------------------------------- every sort form, both tie plans
@pytest.fixture(scope="module", params=list(FORMS))
def form_eng(request):
    e = _context(FORMS[request.param][0], request.param)
    yield e
    e.close()


@gpu
@pytest.mark.parametrize("plan,cid", [("one-sort", c) for c in FORM_CASES] + [("two-sorts", c) for c in FORM_CASES])
def test_family_under_every_sort_form_on_both_tie_plans(form_eng, plan, cid):
    """In the order of the list: the form's fresh context runs the cases on the one-sort plan, the pile-up table (last of
    them) leaves it, and the same cases run again on the two-sort plan the context keeps -- NEAREST k's (end, start) view
    is then a third stable sort, and the by-end view of ``run_sort_two_keys`` ends in the other ping-pong buffer under
    13- to 15-bit buckets (``SortBufs::follow``)."""
    e, case = form_eng, CASES[cid]
    what = (e.form, plan, cid)
    if plan == "two-sorts" and not e.two_sorts:          # (run alone: meet the pile-ups first)
        _nearest(e, CASES[N.PILE_UP], False, None, what, ops=("nearest",))
    assert e.two_sorts == (plan == "two-sorts"), (what, "run this module's tests in their order")
    for signed in (False, True):
        _nearest(e, case, signed, None, what)
    _nearest(e, case, True, case.md, what, ops=("nearest",))
    for k in FORM_KS:
        _nearest_k(e, case, k, k == 3, None, what)
    _group_rows(e, case, what)
    assert e.two_sorts == (plan == "two-sorts" or cid == N.PILE_UP), what
