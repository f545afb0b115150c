"""DISTANCE on the GPU: the per-pair value (HipEngine.distance) and the within-distance join (HipEngine.window_join)
against the golden fixture and the numpy restatement (tests/_distance_ref.py), then the documented recipes through
transpile + execute.  Integers throughout: every comparison is exact."""

import numpy as np
import pytest

import _distance_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pa = pytest.importorskip("pyarrow")

DEV = "cuda:0"
INT32_MAX, INT32_MIN = 2**31 - 1, -2**31
GOLDEN = R.golden()
CASES = GOLDEN["random"]


def _new_engine(env=()):
    from giql_amd.engine import HipEngine

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    with pytest.MonkeyPatch.context() as mp:
        for k, v in env:
            mp.setenv(k, v)
        return HipEngine(0)


@pytest.fixture(scope="module")
def eng():
    e = _new_engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_local():
    """A context that sorts in three stages whenever the density allows (tests/test_sort_stages.py)."""
    e = _new_engine([("GIQL_HIP_LOCAL_MIN_ROWS", "1")])
    yield e
    e.close()


def _t(x, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).to(DEV)


def _side(chrom, start, end, offsets=(0, 0)):
    from giql_amd.engine import DeviceSide

    return DeviceSide(_t(chrom), _t(start), _t(end), offsets[0], offsets[1])


def _pairs(ra, rb):
    return R.sort_pairs(np.stack([ra.cpu().numpy(), rb.cpu().numpy()], 1))


def _values(dist, valid):
    return [int(d) if ok else None for d, ok in zip(dist.cpu().numpy(), valid.cpu().numpy())]


# ------------------------------------------------------------------ HipEngine.distance
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_distance_golden_four_variants(eng, case):
    a, b, _n = R.case_arrays(case)
    sa, sb = _side(*a[:4]), _side(*b[:4])
    p = np.array(case["pairs"], np.int32).reshape(-1, 2)
    ra, rb = _t(p[:, 0]), _t(p[:, 1])
    for variant, (stranded, signed) in R.VARIANTS.items():
        d, v = eng.distance(sa, sb, ra, rb, signed=signed, stranded=stranded,
                            strand_a=_t(a[4]) if stranded else None, strand_b=_t(b[4]) if stranded else None)
        assert d.dtype == torch.int64 and v.dtype == torch.uint8
        assert _values(d, v) == case["values"][variant], variant
    # every pair of the cartesian product: the ones across chromosomes are NULL, in every variant
    ia, ib = np.meshgrid(np.arange(len(case["a"])), np.arange(len(case["b"])), indexing="ij")
    d, v = eng.distance(sa, sb, _t(ia.ravel()), _t(ib.ravel()))
    cross = a[0][ia.ravel()] != b[0][ib.ravel()]
    assert cross.any() and np.array_equal(v.cpu().numpy() == 0, cross) and not d.cpu().numpy()[cross].any()


def test_distance_known_answers(eng):
    for k in GOLDEN["known"]:
        stranded, signed = R.VARIANTS[k["variant"]]
        (ca, s0, e0, t0), (cb, s1, e1, t1) = k["a"], k["b"]
        sa, sb = _side([0], [s0], [e0]), _side([0 if ca == cb else 1], [s1], [e1])
        d, v = eng.distance(sa, sb, _t([0]), _t([0]), signed=signed, stranded=stranded,
                            strand_a=_t([R.STRAND_CODE[t0]]), strand_b=_t([R.STRAND_CODE[t1]]))
        assert _values(d, v) == [k["expected"]], k["source"]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1025])     # 1025 = the rows of one block (256 threads x 4) + 1
def test_distance_sizes(eng, n):
    r = np.random.default_rng(n)
    m = 97
    ac, bc = r.integers(0, 3, m), r.integers(0, 3, m)
    as_, bs = r.integers(0, 500, m), r.integers(0, 500, m)
    ae, be = as_ + r.integers(0, 40, m), bs + r.integers(0, 40, m)
    st_a, st_b = r.integers(0, 5, m), r.integers(0, 5, m)
    ia, ib = r.integers(0, m, n), r.integers(0, m, n)
    for stranded, signed in R.VARIANTS.values():
        d, v = eng.distance(_side(ac, as_, ae), _side(bc, bs, be), _t(ia), _t(ib), signed=signed, stranded=stranded,
                            strand_a=_t(st_a), strand_b=_t(st_b))
        wd, wv = R.distance(ac[ia], as_[ia], ae[ia], bc[ib], bs[ib], be[ib], signed=signed, stranded=stranded,
                            strand_a=st_a[ia], strand_b=st_b[ib])
        assert d.shape == (n,) and np.array_equal(d.cpu().numpy(), wd) and np.array_equal(v.cpu().numpy() != 0, wv)


def test_distance_past_2_31_and_null_validity(eng):
    # rows at both ends of the int32 range; the closed encoding's end + 1 leaves it
    ac, as_, ae = [0, 0, 0, 1], [0, INT32_MIN, INT32_MAX - 1, 5], [1, INT32_MIN + 1, INT32_MAX, 9]
    a = _side(ac, as_, ae, (0, 1))
    b = _side(ac, as_, ae, (0, 1))
    ia, ib = np.meshgrid(np.arange(4), np.arange(4), indexing="ij")
    ia, ib = ia.ravel(), ib.ravel()
    c64 = lambda x: np.asarray(x, np.int64)
    for signed in (False, True):
        d, v = eng.distance(a, b, _t(ia), _t(ib), signed=signed)
        wd, wv = R.distance(c64(ac)[ia], c64(as_)[ia], c64(ae)[ia] + 1, c64(ac)[ib], c64(as_)[ib], c64(ae)[ib] + 1,
                            signed=signed)
        assert np.array_equal(d.cpu().numpy(), wd) and np.array_equal(v.cpu().numpy() != 0, wv)
        assert np.abs(wd).max() == 2**32 - 3 and (wd < 0).any() == signed
    assert int(eng.distance(a, b, _t([0]), _t([2]))[0][0]) == INT32_MAX - 1 - 2 + 1       # 0 .. INT32_MAX: 2^31 - 2
    # NULL: across chromosomes; stranded with '.', '?' or a NULL strand on either side
    d, v = eng.distance(a, b, _t([0, 3, 0]), _t([3, 0, 0]))
    assert _values(d, v) == [None, None, 0]
    one = _side([0] * 5, [10] * 5, [20] * 5)
    two = _side([0] * 5, [30] * 5, [40] * 5)
    codes = _t([R.STRAND_CODE[s] for s in ("+", "-", ".", "?", None)])
    ia, ib = np.meshgrid(np.arange(5), np.arange(5), indexing="ij")
    d, v = eng.distance(one, two, _t(ia.ravel()), _t(ib.ravel()), stranded=True, strand_a=codes, strand_b=codes)
    got = np.array([x if x is not None else 0 for x in _values(d, v)]).reshape(5, 5)
    assert np.array_equal(v.cpu().numpy().reshape(5, 5) != 0, np.pad(np.ones((2, 2), bool), ((0, 3), (0, 3))))
    assert got[:2, :2].tolist() == [[11, 11], [-11, -11]]
    with pytest.raises(ValueError, match="stranded DISTANCE needs strand_a"):
        eng.distance(one, two, _t([0]), _t([0]), stranded=True)


# ------------------------------------------------------------------ HipEngine.window_join
def _window(eng, a, b, n_chrom, n, offs_a=(0, 0), offs_b=(0, 0)):
    """window_join of two ``(chrom, start, end)`` triples (in their tables' encodings) -> sorted pairs; asserts the
    one routed form."""
    got = _pairs(*eng.window_join(_side(*a, offs_a), _side(*b, offs_b), n_chrom, n))
    st = eng.stats()
    assert st["join_form"] == "general" and not st["bucket_join"] and not st["count_fused"] and not st["span_hist"], st
    assert st["n_out"] == got.shape[0]
    return got


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_window_golden(eng, case):
    a, b, n_chrom = R.case_arrays(case)
    for n in GOLDEN["within_n"]:
        got = _window(eng, a[:3], b[:3], n_chrom, n, a[3], b[3])       # non-canonical encodings through the offsets
        assert got.tolist() == case["within"][str(n)], n
    st = eng.stats()
    assert st["span"] < 3 * 6000        # N = 2^40 did not inflate the axis: each chromosome's range + 2
    # N = 0: the multiset of the INNER join of the same sides
    sa, sb = _side(*a[:4]), _side(*b[:4])
    assert np.array_equal(_pairs(*eng.window_join(sa, sb, n_chrom, 0)), _pairs(*eng.inner_join(sa, sb, n_chrom)))
    assert np.array_equal(_pairs(*eng.window_join(sa, sb, n_chrom, 0)),
                          R.overlap_pairs(*R.canonical(a), *R.canonical(b)))


def test_window_book_ended_zero_length_and_the_clamp(eng):
    # book-ended rows: out at N = 0, in at N = 1 (distance 1), on either end
    a = ([0, 0], [100, 300], [200, 400])
    b = ([0, 0, 0], [200, 250, 401], [250, 300, 402])
    assert _window(eng, a, b, 1, 0).tolist() == []
    assert _window(eng, a, b, 1, 1).tolist() == [[0, 0], [1, 1]]
    assert _window(eng, a, b, 1, 2).tolist() == [[0, 0], [1, 1], [1, 2]]
    # zero-length rows on either side; [3,5) against [0,0) at N = 10 is the counter-example to a clamp at 0
    assert _window(eng, ([0], [3], [5]), ([0], [0], [0]), 1, 10).tolist() == [[0, 0]]
    assert _window(eng, ([0], [3], [5]), ([0], [0], [0]), 1, 3).tolist() == []
    assert _window(eng, ([0], [3], [5]), ([0], [0], [0]), 1, 4).tolist() == [[0, 0]]
    assert _window(eng, ([0], [0], [0]), ([0], [3], [5]), 1, 4).tolist() == [[0, 0]]
    r = np.random.default_rng(5)
    m = 300
    ac, bc = r.integers(0, 2, m), r.integers(0, 2, m)
    as_, bs = r.integers(-50, 400, m), r.integers(-50, 400, m)
    ae = as_ + np.where(r.random(m) < 0.4, 0, r.integers(0, 30, m))         # many zero-length rows, negative coordinates
    be = bs + np.where(r.random(m) < 0.4, 0, r.integers(0, 30, m))
    for n in (0, 1, 7):
        got = _window(eng, (ac, as_, ae), (bc, bs, be), 2, n)
        assert np.array_equal(got, R.window_pairs(ac, as_, ae, bc, bs, be, n)) and got.shape[0] > 100
        st = eng.stats()
        assert st["n_irregular_b"] == int((bs == be).sum())
        assert st["n_irregular_a"] == (int((as_ == ae).sum()) if n == 0 else 0)


def test_window_chromosome_boundaries_absent_chromosomes_empty_sides_and_a_huge_n(eng):
    # the last row of chromosome 0 and the first row of chromosome 1 are neighbours on the linear axis
    a = ([0, 1, 2], [990, 0, 5], [1000, 10, 6])
    b = ([1, 0, 1, 3], [0, 995, 12, 5], [3, 1000, 20, 6])
    for n in (0, 1, 5, 100, 1 << 40):
        got = _window(eng, a, b, 4, n)
        assert np.array_equal(got, R.window_pairs(*a, *b, n))
        assert all(a[0][i] == b[0][j] for i, j in got.tolist())
    assert _window(eng, a, b, 4, 1 << 40).tolist() == [[0, 1], [1, 0], [1, 2]]   # chromosomes 2 / 3: one side only
    assert eng.stats()["span"] <= (1000 - 990 + 3) + (20 - 0 + 3) + 4 + 4     # no span error, no inflation at 2^40
    assert _window(eng, a, b, 4, (1 << 63) - 1).tolist() == [[0, 1], [1, 0], [1, 2]]
    empty = ([], [], [])
    for x, y in ((empty, b), (a, empty), (empty, empty)):
        assert _window(eng, x, y, 4, 9).shape == (0, 2)
    with pytest.raises(ValueError, match="max_distance must be >= 0"):
        eng.window_join(_side(*a), _side(*b), 4, -1)


def test_window_inverted_rows_are_a_value_error_naming_the_side(eng):
    good = ([0, 0], [1, 5], [4, 9])
    bad = ([0, 0], [1, 9], [4, 5])
    from giql_amd.engine import InvertedRows

    # the side comes from the library's stats (n_irregular_x = -1), the message says it as well
    for x, y, sides in ((bad, good, ("a",)), (good, bad, ("b",)), (bad, bad, ("a", "b"))):
        with pytest.raises(ValueError, match=f"side {sides[0]} has a row with start > end") as ei:
            eng.window_join(_side(*x), _side(*y), 1, 3)
        assert isinstance(ei.value, InvertedRows) and ei.value.sides == sides
        st = eng.stats()
        assert (st["n_irregular_a"] == -1, st["n_irregular_b"] == -1) == ("a" in sides, "b" in sides)
    # inverted only in the declared encoding: [5, 4] 0-based closed is the zero-length [5, 5)
    assert _window(eng, ([0], [5], [4]), ([0], [5], [9]), 1, 1, offs_a=(0, 1)).tolist() == [[0, 0]]
    # the context goes on working after the refusal
    assert _window(eng, good, good, 1, 0).tolist() == [[0, 0], [1, 1]]


@pytest.mark.parametrize("uniform", [False, True], ids=["variable", "uniform"])
@pytest.mark.parametrize("which", ["default", "local"])
def test_window_on_both_sort_forms_and_uniform_lengths(eng, eng_local, which, uniform):
    """Tables dense enough for the three-stage sort (about 1,000 rows per 65,536 positions): the same one form,
    whatever the sort underneath, and a side of ONE length does not reach the fixed-length plan."""
    e = eng if which == "default" else eng_local
    r = np.random.default_rng(11)
    m = 2000
    ac, bc = r.integers(0, 2, m), r.integers(0, 2, m)
    as_, bs = r.integers(0, 60000, m), r.integers(0, 60000, m)
    ae = as_ + r.integers(0, 120, m)
    be = bs + (50 if uniform else r.integers(0, 120, m))
    for n in (0, 25):
        got = _window(e, (ac, as_, ae), (bc, bs, be), 2, n)
        assert np.array_equal(got, R.window_pairs(ac, as_, ae, bc, bs, be, n)) and got.shape[0] > 1000
        assert e.stats()["sort_local"] == (which == "local")
    # a plain INTERSECTS join on the same context afterwards takes the forms it always took
    sa, sb = _side(ac, as_, ae + 1), _side(bc, bs, be + 1)
    assert np.array_equal(_pairs(*e.inner_join(sa, sb, 2)), R.overlap_pairs(ac, as_, ae + 1, bc, bs, be + 1))
    assert e.stats()["join_form"] == ("uniform_b" if uniform else "general")


def test_window_span_error_takes_the_chromosome_group_fallback(eng):
    from giql_amd import _lib

    # two chromosomes that each fill most of the 32-bit axis
    a = ([0, 0, 1, 1], [0, INT32_MAX - 10, INT32_MIN, INT32_MAX - 100], [10, INT32_MAX, INT32_MIN + 5, INT32_MAX - 90])
    b = ([0, 1, 1, 0], [12, INT32_MIN + 8, INT32_MAX - 85, INT32_MAX - 30], [20, INT32_MIN + 9, INT32_MAX - 80, INT32_MAX - 20])
    with pytest.raises(_lib.GiqlHipError) as ei:
        eng._window_once(_side(*a), _side(*b), 2, 5)
    assert ei.value.code == _lib.GIQL_ERR_SPAN
    for n in (0, 3, 10, 1 << 40):
        got = _pairs(*eng.window_join(_side(*a), _side(*b), 2, n))
        assert np.array_equal(got, R.window_pairs(*a, *b, n))
    assert got.shape[0] == 8


# ------------------------------------------------------------------ execute()
def _table(rows):
    return pa.table({"chrom": pa.array([r[0] for r in rows], pa.string()),
                     "start": pa.array([r[1] for r in rows], pa.int32()),
                     "end": pa.array([r[2] for r in rows], pa.int32()),
                     "strand": pa.array([r[3] for r in rows], pa.string()),
                     "name": pa.array([f"n{i:03d}" for i in range(len(rows))], pa.string()),
                     "score": pa.array([i % 7 for i in range(len(rows))], pa.int32())})


def _giql_tables(case):
    from giql_amd.table import Table

    return [Table("features_a", coordinate_system=case["enc_a"][0], interval_type=case["enc_a"][1]),
            Table("features_b", coordinate_system=case["enc_b"][0], interval_type=case["enc_b"][1])]


@pytest.mark.parametrize("case", CASES[:4], ids=[c["id"] for c in CASES[:4]])
def test_execute_the_documented_recipes(eng, case):
    from giql_amd.execute import execute

    data = {"features_a": _table(case["a"]), "features_b": _table(case["b"])}
    tables = _giql_tables(case)
    value = dict(zip(map(tuple, case["pairs"]), case["values"]["plain"]))
    want = sorted((f"n{i:03d}", value[(i, j)], f"n{j:03d}") for i, j in case["within"]["50"])
    recipes = [
        "SELECT a.name, b.name AS b_name, DISTANCE(a.interval, b.interval) AS dist FROM features_a a "
        "CROSS JOIN features_b b WHERE a.chrom = b.chrom AND DISTANCE(a.interval, b.interval) <= 50",
        "SELECT a.name, b.name AS b_name, DISTANCE(a.interval, b.interval) AS dist FROM features_a a "
        "JOIN features_b b ON DISTANCE(b.interval, a.interval) < 51",
        "SELECT a.name, b.name AS b_name, DISTANCE(b.interval, a.interval) AS dist FROM features_a a, features_b b "
        "WHERE DISTANCE(a.interval, b.interval) <= 50",
    ]
    for q in recipes:
        out = execute(q + " ORDER BY a.name, dist", data, eng, giql_tables=tables)
        assert out.schema.field("dist").type == pa.int64() and out.column_names == ["name", "b_name", "dist"]
        rows = list(zip(out["name"].to_pylist(), out["dist"].to_pylist(), out["b_name"].to_pylist()))
        assert sorted(rows) == want
        assert [(r[0], r[1]) for r in rows] == sorted((r[0], r[1]) for r in rows)       # ORDER BY a.name, dist
    ra, rb = execute(recipes[0], data, eng, giql_tables=tables, return_indices=True)
    assert R.sort_pairs(np.stack([ra, rb], 1)).tolist() == case["within"]["50"]
    # a residual beside the predicate; < 0 is an ordinary empty result; DISTINCT and LIMIT on the value
    out = execute(recipes[1] + " AND a.score > 2 AND b.score <= a.score", data, eng, giql_tables=tables)
    keep = [(i, j) for i, j in case["within"]["50"] if i % 7 > 2 and j % 7 <= i % 7]
    assert sorted(zip(out["name"].to_pylist(), out["b_name"].to_pylist())) == sorted((f"n{i:03d}", f"n{j:03d}") for i, j in keep)
    out = execute("SELECT a.name FROM features_a a, features_b b WHERE DISTANCE(a.interval, b.interval) < 0", data, eng,
                  giql_tables=tables)
    assert out.num_rows == 0
    out = execute("SELECT DISTINCT DISTANCE(a.interval, b.interval) AS d FROM features_a a, features_b b "
                  "WHERE DISTANCE(a.interval, b.interval) <= 50 ORDER BY d LIMIT 3", data, eng, giql_tables=tables)
    assert out["d"].to_pylist() == sorted({v for _n, v, _m in want})[:3]
    with pytest.raises(ValueError, match="run on one device"):
        execute(recipes[0], data, giql_tables=tables, devices=[0, 0])


def test_execute_distance_beside_intersects_stranded_nulls_and_pinned_tables(eng):
    from giql_amd.execute import execute, pin

    case = CASES[4]         # (its pairs within 50 hold NULL, positive and negative stranded values)
    data = {"features_a": _table(case["a"]), "features_b": _table(case["b"])}
    tables = _giql_tables(case)
    a, b, _n = R.case_arrays(case)
    over = R.overlap_pairs(*R.canonical(a), *R.canonical(b)).tolist()
    out = execute("SELECT a.name, b.name AS b_name, DISTANCE(a.interval, b.interval) AS d FROM features_a a "
                  "JOIN features_b b ON a.interval INTERSECTS b.interval", data, eng, giql_tables=tables)
    assert out.num_rows == len(over) > 0 and set(out["d"].to_pylist()) == {0} and out["d"].null_count == 0
    # the stranded, signed value with B as the CASE's first operand: NULLs where a strand is '.', '?' or NULL
    value = {}
    for (i, j) in case["within"]["50"]:
        d, v = R.distance(*[x[[j]] for x in R.canonical(b)], *[x[[i]] for x in R.canonical(a)], signed=True,
                          stranded=True, strand_a=b[4][[j]], strand_b=a[4][[i]])
        value[(f"n{i:03d}", f"n{j:03d}")] = int(d[0]) if v[0] else None
    out = execute("SELECT a.name, b.name AS b_name, DISTANCE(b.interval, a.interval, stranded := true, signed := true) "
                  "AS d FROM features_a a JOIN features_b b ON DISTANCE(a.interval, b.interval) <= 50", data, eng,
                  giql_tables=tables)
    got = dict(zip(zip(out["name"].to_pylist(), out["b_name"].to_pylist()), out["d"].to_pylist()))
    assert got == value and out["d"].null_count == sum(v is None for v in value.values()) > 0
    assert any(v is not None and v < 0 for v in value.values())
    # pinned tables work as plain tables
    pinned = {k: pin(t, index=True) for k, t in data.items()}      # (an index is offered and not used)
    q = ("SELECT a.name, b.name AS b_name FROM features_a a JOIN features_b b ON DISTANCE(a.interval, b.interval) <= 2")
    out = execute(q, pinned, eng, giql_tables=tables)
    assert sorted(zip(out["name"].to_pylist(), out["b_name"].to_pylist())) == \
        sorted((f"n{i:03d}", f"n{j:03d}") for i, j in case["within"]["2"])


def test_execute_names_the_table_with_an_inverted_row(eng):
    from giql_amd.execute import execute

    good = _table([["chr1", 1, 4, "+"], ["chr1", 5, 9, "-"]])
    bad = _table([["chr1", 1, 4, "+"], ["chr1", 9, 5, "-"]])
    q = "SELECT a.name FROM features_a a JOIN features_b b ON DISTANCE(a.interval, b.interval) <= 3"
    with pytest.raises(ValueError, match="table 'features_b' has a row with start > end"):
        execute(q, {"features_a": good, "features_b": bad}, eng, giql_tables=["features_a", "features_b"])
    with pytest.raises(ValueError, match="table 'features_a' has a row with start > end"):
        execute(q, {"features_a": bad, "features_b": good}, eng, giql_tables=["features_a", "features_b"])
    with pytest.raises(ValueError, match="table 'features_a' and 'features_b' has a row with start > end"):
        execute(q, {"features_a": bad, "features_b": bad}, eng, giql_tables=["features_a", "features_b"])
