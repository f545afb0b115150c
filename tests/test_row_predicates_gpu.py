"""SEMI / ANTI / COUNT over CONTAINS, WITHIN and DISTANCE <= N on the GPU (HipEngine.semi_anti_pred / count_pred,
execute(row_predicates=True)): the two golden fixtures reduced per left row, every path case of the candidate-tile
walk, a seeded DISTANCE table for the rank difference, hand-made edges, the chromosome-group fallback, the plan
protocol and execute() against the reduction of its own INNER form.  Integers throughout: every comparison is
exact."""

import ctypes

import numpy as np
import pytest

import _contain_ref as CR
import _distance_ref as DR
import _rows_ref as RR

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pa = pytest.importorskip("pyarrow")

DEV = "cuda:0"
INT32_MIN, INT32_MAX = -(2**31), 2**31 - 1


@pytest.fixture(scope="module")
def eng():
    from giql_amd.engine import HipEngine

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    e = HipEngine(0)
    yield e
    e.close()


def _side(chrom, start, end, offsets=(0, 0)):
    from giql_amd.engine import DeviceSide

    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.int32)).to(DEV)
    return DeviceSide(t(chrom), t(start), t(end), offsets[0], offsets[1])


def _check(eng, a, b, n_chrom, predicate, pairs, max_distance=None, form=None, what="", single=True):
    """SEMI, ANTI and COUNT of ``a <predicate> b`` against the reduction of ``pairs``; returns the counts.
    ``single=False``: the call runs group by group, the context's stats are the last group's."""
    semi, anti, counts = RR.reduce_pairs(pairs, a.n)
    got = eng.semi_anti_pred(a, b, n_chrom, predicate, False, max_distance).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, semi), (what, predicate, "semi")
    assert (eng.stats()["n_out"] == semi.size or not single) and eng.stats()["join_form"] == "general"
    got = eng.semi_anti_pred(a, b, n_chrom, predicate, True, max_distance).cpu().numpy()
    assert np.array_equal(got, anti), (what, predicate, "anti")
    got = eng.count_pred(a, b, n_chrom, predicate, max_distance)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), counts), (what, predicate, "count")
    if form is not None:
        assert eng.stats()["join_form"] == form, (what, predicate, eng.stats())
    return got


# ------------------------------------------------------------------ 1, 2: the golden fixtures
CT_CASES = CR.golden_cases()
GOLDEN = DR.golden()


@pytest.mark.parametrize("case", CT_CASES, ids=[c["id"] for c in CT_CASES])
def test_containment_fixture(eng, case):
    ac, as_, ae, offs_a, bc, bs, be, offs_b, n_chrom = CR.case_arrays(case)
    a, b = _side(ac, as_, ae, offs_a), _side(bc, bs, be, offs_b)     # each table in its declared encoding
    _check(eng, a, b, n_chrom, "contains", case["contains"], what=case["id"])
    _check(eng, a, b, n_chrom, "within", case["within"], what=case["id"])


@pytest.mark.parametrize("case", GOLDEN["random"], ids=[c["id"] for c in GOLDEN["random"]])
def test_distance_fixture_random(eng, case):
    a, b, n_chrom = DR.case_arrays(case)
    sa, sb = _side(*a[:4]), _side(*b[:4])
    for n in GOLDEN["within_n"]:
        _check(eng, sa, sb, n_chrom, "within_distance", case["within"][str(n)], n, "general", (case["id"], n))
    assert eng.stats()["span"] < 3 * 6000        # N = 2^40 did not inflate the axis


def test_distance_fixture_known(eng):
    for k in GOLDEN["known"]:
        (ca, s0, e0, _t0), (cb, s1, e1, _t1) = k["a"], k["b"]
        a = ([0], [s0], [e0])
        b = ([0 if ca == cb else 1], [s1], [e1])
        for n in GOLDEN["within_n"]:
            want = DR.window_pairs(*a, *b, n)
            if k["variant"] == "plain":       # the fixture's own value says the same
                assert (want.shape[0] == 1) == (k["expected"] is not None and k["expected"] <= n), k["source"]
            _check(eng, _side(*a), _side(*b), 2, "within_distance", want, n, "general", (k["source"], n))


# ------------------------------------------------------------------ 3: the candidate-tile walk's path cases
@pytest.mark.parametrize("cid", list(CR.PATH_CASES))
def test_path_cases(eng, cid):
    case = CR.path_case(cid)
    o, i = _side(*case.outer), _side(*case.inner)
    want = case.want                                            # (outer row, inner row), R.truth
    uniform = cid.startswith("uniform") or cid == "sort-uniform"
    per_outer = _check(eng, o, i, case.n_chrom, "contains", want, form="uniform_b" if uniform else "general", what=cid)
    _check(eng, i, o, case.n_chrom, "within", RR.transpose(want), form="general", what=cid)
    st = eng.stats()
    assert st["n_irregular_a"] == int((case.inner[2] <= case.inner[1]).sum())
    assert st["n_irregular_b"] == int((case.outer[2] <= case.outer[1]).sum())
    if cid == "straddle":       # integer atomics: a second run gives the same bits
        again = eng.count_pred(o, i, case.n_chrom, "contains")
        assert torch.equal(per_outer, again)


# ------------------------------------------------------------------ 4: the rank-difference count
def _distance_table():
    r = np.random.default_rng(4099)
    n = 4099
    sides = []
    for _ in range(2):
        c = r.integers(0, 3, n)
        s = r.integers(0, 3_000_000, n)
        e = s + r.integers(1, 5000, n)
        z = r.choice(n, 50, replace=False)
        e[z] = s[z]                                             # 50 zero-length rows a side
        sides.append((c, s, e))
    return sides


def test_seeded_distance_table(eng):
    a, b = _distance_table()
    sa, sb = _side(*a), _side(*b)
    for n in (0, 1, 1000, 1 << 40):
        want = RR.window_counts(*a, *b, n)
        got = eng.count_pred(sa, sb, 3, "within_distance", n)
        st = eng.stats()
        assert np.array_equal(got.cpu().numpy(), want), n
        assert st["join_form"] == "general" and st["n_irregular_b"] == 50 and st["n_irregular_a"] == (50 if n == 0 else 0)
        ids = np.arange(want.size)
        assert np.array_equal(eng.semi_anti_pred(sa, sb, 3, "within_distance", False, n).cpu().numpy(), ids[want > 0])
        assert np.array_equal(eng.semi_anti_pred(sa, sb, 3, "within_distance", True, n).cpu().numpy(), ids[want == 0])
    assert (want == np.bincount(b[0], minlength=3)[a[0]]).all()       # N = 2^40: every row of the chromosome
    zero = a[2] == a[1]
    assert (RR.window_counts(*a, *b, 0)[zero] > 0).any()               # a zero-length row with a neighbour at N = 0


# ------------------------------------------------------------------ 5: hand-made edges
def test_zero_length_and_inverted_rows_follow_the_literal_predicate(eng):
    p = _side([0], [5], [5])
    for predicate in ("contains", "within"):
        _check(eng, p, p, 1, predicate, [[0, 0]], what="[5,5) and [5,5)")
    # inverted rows on both sides: [9,4) CONTAINS [9,4), [9,4) CONTAINS [10,3), [2,8) CONTAINS [6,1) (6 >= 2, 1 <= 8)
    a = ([0, 0, 0, 0], [9, 2, 7, 5], [4, 8, 7, 1])
    b = ([0, 0, 0, 0, 0], [9, 10, 6, 3, 7], [4, 3, 1, 9, 7])
    want = CR.contain_pairs(*a, *b)
    assert [0, 0] in want.tolist() and [0, 1] in want.tolist() and [1, 2] in want.tolist()
    _check(eng, _side(*a), _side(*b), 1, "contains", want)
    _check(eng, _side(*b), _side(*a), 1, "within", RR.transpose(want))
    _check(eng, _side(*a), _side(*b), 1, "within", RR.transpose(CR.contain_pairs(*b, *a)))


def test_distance_zero_length_rows_and_the_clamp(eng):
    _check(eng, _side([0], [5], [5]), _side([0], [3], [8]), 1, "within_distance", [[0, 0]], 0)   # distance 0
    a, b = _side([0], [3], [5]), _side([0], [0], [0])           # distance 4: the clamp example
    _check(eng, a, b, 1, "within_distance", [[0, 0]], 10)
    _check(eng, a, b, 1, "within_distance", [], 3)
    _check(eng, a, b, 1, "within_distance", [[0, 0]], 4)
    # book-ended rows have distance 1; zero-length rows on both sides at one point have distance 1 as well
    _check(eng, _side([0, 0], [0, 7], [5, 7]), _side([0, 0], [5, 7], [9, 7]), 1, "within_distance",
           DR.window_pairs([0, 0], [0, 7], [5, 7], [0, 0], [5, 7], [9, 7], 0), 0)
    for n in (0, 1):
        _check(eng, _side([0, 0], [0, 7], [5, 7]), _side([0, 0], [5, 7], [9, 7]), 1, "within_distance",
               DR.window_pairs([0, 0], [0, 7], [5, 7], [0, 0], [5, 7], [9, 7], n), n)


def test_chromosomes_do_not_leak(eng):
    # the query sits on chromosome 1 at [1000, 2000); chromosome 2 (later) holds only smaller coordinates, chromosome
    # 0 (earlier) only larger ones, chromosome 3 is absent from B
    a = ([1, 1, 3, 0], [1000, 1500, 10, 9000], [2000, 1600, 20, 9001])
    b = ([2, 2, 0, 0, 1], [0, 1200, 5000, 1000, 1400], [5000, 1300, 9999, 2000, 1700])
    sa, sb = _side(*a), _side(*b)
    for predicate, pairs in (("contains", CR.contain_pairs(*a, *b)),
                             ("within", RR.transpose(CR.contain_pairs(*b, *a)))):
        _check(eng, sa, sb, 4, predicate, pairs)
    assert CR.contain_pairs(*a, *b).tolist() == [[0, 4]] and CR.contain_pairs(*b, *a).tolist() == [[2, 3], [4, 1]]
    for n in (0, 50, 1 << 40):
        _check(eng, sa, sb, 4, "within_distance", DR.window_pairs(*a, *b, n), n)
    assert DR.window_pairs(*a, *b, 1 << 40).tolist() == [[0, 4], [1, 4], [3, 2], [3, 3]]


def test_empty_sides_and_a_negative_bound(eng):
    a, none = _side([0, 0], [1, 5], [4, 9]), _side([], [], [])
    for predicate, md in (("contains", None), ("within", None), ("within_distance", 3)):
        _check(eng, a, none, 1, predicate, [], md)
        assert sum(eng.stats()["phase_launches"].values()) == 0          # an empty right side: nothing is spanned or sorted
        assert eng.semi_anti_pred(none, a, 1, predicate, True, md).numel() == 0
        assert eng.count_pred(none, a, 1, predicate, md).numel() == 0
        assert sum(eng.stats()["phase_launches"].values()) == 0
    _check(eng, a, a, 1, "within_distance", [], -1)                      # `< 0`: nothing qualifies
    with pytest.raises(ValueError):
        eng.count_pred(a, a, 1, "within_distance", -2)
    with pytest.raises(ValueError):
        eng.semi_anti_pred(a, a, 1, "overlaps", False)


def test_distance_refuses_inverted_rows_naming_the_side(eng):
    from giql_amd.engine import InvertedRows

    good, bad = _side([0, 0], [1, 5], [4, 9]), _side([0, 0], [1, 9], [4, 5])
    for a, b, sides in ((bad, good, ("a",)), (good, bad, ("b",)), (bad, bad, ("a", "b"))):
        for md in (0, 7, -1):
            with pytest.raises(InvertedRows) as ei:
                eng.semi_anti_pred(a, b, 1, "within_distance", False, md)
            assert ei.value.sides == sides
            with pytest.raises(InvertedRows) as ei:
                eng.count_pred(a, b, 1, "within_distance", md)
            assert ei.value.sides == sides
    _check(eng, bad, good, 1, "contains", CR.contain_pairs([0, 0], [1, 9], [4, 5], [0, 0], [1, 5], [4, 9]))


# ------------------------------------------------------------------ 6: past the 32-bit axis
def test_the_chromosome_group_fallback(eng):
    from giql_amd import _lib

    r = np.random.default_rng(232)
    n = 300

    def table():
        c = r.integers(0, 2, n)
        s = np.where(r.random(n) < 0.5, r.integers(INT32_MIN, INT32_MIN + 100000, n),
                     r.integers(INT32_MAX - 101000, INT32_MAX - 1000, n))
        return c, s, s + r.integers(0, 900, n)

    a, b = table(), table()
    sa, sb = _side(*a), _side(*b)
    with pytest.raises(_lib.GiqlHipError) as ei:
        eng._count_pred_once(sa, sb, 2, _lib.ROWPRED_CONTAINS, 0)
    assert ei.value.code == _lib.GIQL_ERR_SPAN
    with pytest.raises(_lib.GiqlHipError) as ei:
        eng._semi_anti_pred_once(sa, sb, 2, _lib.ROWPRED_DISTANCE, 5, False)
    assert ei.value.code == _lib.GIQL_ERR_SPAN
    ct = CR.contain_pairs(*a, *b)
    assert ct.shape[0] > 20 and 0 < np.unique(ct[:, 0]).size < n
    _check(eng, sa, sb, 2, "contains", ct, single=False)
    _check(eng, sa, sb, 2, "within", RR.transpose(CR.contain_pairs(*b, *a)), single=False)
    for md in (0, 40, 1 << 40):
        want = RR.window_counts(*a, *b, md)
        assert np.array_equal(eng.count_pred(sa, sb, 2, "within_distance", md).cpu().numpy(), want)
        assert md > 40 or 0 < (want > 0).sum() < n
        ids = np.arange(n)
        assert np.array_equal(eng.semi_anti_pred(sa, sb, 2, "within_distance", False, md).cpu().numpy(), ids[want > 0])
        assert np.array_equal(eng.semi_anti_pred(sa, sb, 2, "within_distance", True, md).cpu().numpy(), ids[want == 0])


# ------------------------------------------------------------------ 7: the plan protocol
def test_the_new_calls_drop_a_plan_held_in_the_context(eng):
    from giql_amd import _lib

    a = _side([0, 0, 0], [0, 10, 20], [15, 30, 25])
    b = _side([0, 0, 0, 0], [2, 12, 21, 22], [9, 28, 24, 40])
    buf = [torch.empty(16, dtype=torch.int32, device=DEV) for _ in range(2)]
    L, h, st = eng._L, eng._h, eng._stream()
    calls = [lambda: eng.semi_anti_pred(a, b, 1, "contains", False), lambda: eng.count_pred(a, b, 1, "within"),
             lambda: eng.count_pred(a, b, 1, "within_distance", 3), lambda: eng.semi_anti_pred(a, b, 1, "within_distance", True, 0)]
    for call in calls:
        n = eng.inner_plan(a, b, 1)
        assert 0 < n <= 16
        call()
        assert L.giql_hip_inner_fill_dev(h, buf[0].data_ptr(), buf[1].data_ptr(), 16, st) == _lib.GIQL_ERR_STATE
        n = eng.contain_plan(a, b, 1)
        assert 0 < n <= 16
        eng.contain_fill(buf[0], buf[1])                   # the plan is there until the next launching call
        call()
        assert L.giql_hip_contain_fill_dev(h, buf[0].data_ptr(), buf[1].data_ptr(), 16, st) == _lib.GIQL_ERR_STATE
    bad = ctypes.c_int64(0)
    ca, cb = a.c_struct(), b.c_struct()
    assert L.giql_hip_semi_anti_pred_dev(h, ca, cb, 1, 4, 0, 0, buf[0].data_ptr(), ctypes.byref(bad), st) == _lib.GIQL_ERR_INVALID
    assert L.giql_hip_count_pred_dev(h, ca, cb, 1, 3, -2, None, st) == _lib.GIQL_ERR_INVALID
    chrom = _side([0, 3], [0, 5], [9, 8]).c_struct()
    assert L.giql_hip_semi_anti_pred_dev(h, chrom, cb, 1, 1, 0, 0, buf[0].data_ptr(), ctypes.byref(bad), st) == _lib.GIQL_ERR_CHROM


# ------------------------------------------------------------------ 8: execute()
def _tables():
    r = np.random.default_rng(88)

    def table(n, seed_len):
        c = r.integers(0, 3, n)
        s = r.integers(0, 12000, n)
        e = s + r.integers(0, seed_len, n)
        return pa.table({"chrom": pa.array([f"chr{x + 1}" for x in c], pa.string()), "start": pa.array(s, pa.int32()),
                         "end": pa.array(e, pa.int32()), "name": pa.array([f"r{i:04d}" for i in range(n)], pa.string()),
                         "score": pa.array(r.integers(0, 7, n), pa.int32())})

    return {"ta": table(400, 150), "tb": table(500, 150)}


PREDS = {"contains": "a.interval CONTAINS b.interval", "within": "a.interval WITHIN b.interval",
         "distance": "DISTANCE(a.interval, b.interval) <= 7"}


@pytest.mark.parametrize("word", list(PREDS))
def test_execute_equals_the_reduction_of_its_inner_form(eng, word):
    from giql_amd.execute import execute
    from giql_amd.shape import HipDeclined

    data = _tables()
    on = PREDS[word]
    n_a = data["ta"].num_rows
    score_a = data["ta"].column("score").to_numpy()
    ids = np.arange(n_a)

    def inner(extra=""):
        ra, rb = execute(f"SELECT a.name, b.name AS bn FROM ta a JOIN tb b ON {on}{extra}", data, eng, return_indices=True)
        return np.stack([ra, rb], 1)

    def rows(kind, extra="", where="", **kw):
        q = f"SELECT a.name FROM ta a {kind} JOIN tb b ON {on}{extra}{where}"
        with pytest.raises(HipDeclined):
            execute(q, data, eng, return_indices=True)
        return execute(q, data, eng, return_indices=True, row_predicates=True, **kw)

    semi, anti, counts = RR.reduce_pairs(inner(), n_a)
    assert semi.size > 10 and anti.size > 10 and counts.max() >= 2
    assert np.array_equal(rows("SEMI"), semi) and np.array_equal(rows("ANTI"), anti)
    for extra in (" AND a.score > 2", " AND b.score < 4", " AND a.score >= b.score"):     # left-only, right-only, two-sided
        s, a, _ = RR.reduce_pairs(inner(extra), n_a)
        assert 0 < s.size < semi.size
        assert np.array_equal(rows("SEMI", extra), s) and np.array_equal(rows("ANTI", extra), a), extra
    keep = score_a != 3                                   # WHERE filters the surviving left rows
    assert np.array_equal(rows("SEMI", where=" WHERE a.score <> 3"), semi[keep[semi]])
    assert np.array_equal(rows("ANTI", where=" WHERE a.score <> 3"), anti[keep[anti]])
    out = execute(f"SELECT a.name FROM ta a SEMI JOIN tb b ON {on} ORDER BY a.name", data, eng, row_predicates=True)
    assert out.column("name").to_pylist() == [f"r{i:04d}" for i in semi]
    # the -v shortcut needs both switches
    v = f"SELECT a.name FROM ta a LEFT JOIN tb b ON {on} WHERE b.chrom IS NULL"
    assert np.array_equal(execute(v, data, eng, return_indices=True, outer_joins=True, row_predicates=True), anti)
    with pytest.raises(HipDeclined):
        execute(v, data, eng, return_indices=True, row_predicates=True)
    # count_overlaps: per left row, and with its GROUP BY projected
    cq = f"SELECT a.chrom, a.start, a.end, COUNT(b.start) AS n FROM ta a LEFT JOIN tb b ON {on} GROUP BY a.chrom, a.start, a.end"
    with pytest.raises(HipDeclined):
        execute(cq, data, eng)
    assert np.array_equal(np.asarray(execute(cq, data, eng, return_indices=True, row_predicates=True)), counts)
    out = execute(cq, data, eng, row_predicates=True)
    assert out.column_names == ["chrom", "start", "end", "n"]
    want = {}
    for i, key in enumerate(zip(data["ta"].column("chrom").to_pylist(), data["ta"].column("start").to_pylist(),
                                data["ta"].column("end").to_pylist())):
        want[key] = want.get(key, 0) + int(counts[i])
    got = dict(zip(zip(out.column("chrom").to_pylist(), out.column("start").to_pylist(), out.column("end").to_pylist()),
                   out.column("n").to_pylist()))
    assert got == want
    with pytest.raises(NotImplementedError):
        execute(cq, data, devices=[0, 1], row_predicates=True)


def test_execute_names_the_table_with_an_inverted_row(eng):
    from giql_amd.execute import execute

    data = _tables()
    bad = data["tb"].set_column(2, "end", pa.array(np.where(np.arange(500) == 7, -5, data["tb"].column("end").to_numpy()), pa.int32()))
    for q in (f"SELECT a.name FROM ta a SEMI JOIN tb b ON {PREDS['distance']}",
              f"SELECT a.chrom, a.start, a.end, COUNT(b.start) AS n FROM ta a LEFT JOIN tb b ON {PREDS['distance']} "
              "GROUP BY a.chrom, a.start, a.end"):
        with pytest.raises(ValueError, match="table 'tb' has a row with start > end"):
            execute(q, {"ta": data["ta"], "tb": bad}, eng, row_predicates=True)
