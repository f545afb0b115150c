"""Literal range sets on the GPU: ``HipEngine.range_set_any`` against tests/_range_set_ref.py (a NumPy restatement in
three-valued logic, itself checked against sqlite3 in tests/test_range_sets.py) and ``execute(..., range_sets=True)``
against every case of tests/golden/range_sets.json.  Everything compares with ``==``: the kernel computes no number,
only flags."""
import json
import os

import numpy as np
import pytest

import _range_set_ref as ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "range_sets.json")))
TILE = 1024   # RSET_TILE (giql_amd/csrc/range_set_kernels.hip.h): rows per tile, four per thread
OPS = ("intersects", "contains", "within")


@pytest.fixture(scope="module")
def eng():
    from giql_amd.engine import HipEngine

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    e = HipEngine(0)
    yield e
    e.close()


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _as_bounds(op, ranges):
    """Canonical ``(code, lo, hi)`` ranges as a set of ``range_set_any`` (a 0-based half-open table: no shift)."""
    codes = [r[0] for r in ranges]
    lo, hi = [r[1] for r in ranges], [r[2] for r in ranges]
    return (op, codes, hi, lo) if op == "intersects" else (op, codes, lo, hi)


def _check(eng, chrom, start, end, sets, valid=(None, None, None)):
    """Run every set in one call and compare both byte arrays with the reference."""
    n = len(chrom)
    ok = [np.ones(n, bool) if v is None else np.asarray(v, bool) for v in valid]
    got = eng.range_set_any(_dev(chrom.astype(np.int32)), _dev(start.astype(np.int32)), _dev(end.astype(np.int32)), sets,
                            valid=[None if v is None else _dev(np.asarray(v, np.uint8)) for v in valid])
    assert len(got) == len(sets)
    for (op, codes, on_start, on_end), (value, known) in zip(sets, got):
        want_value, want_known = ref.any_over_bounds(op, chrom, start, end, ok[0], ok[1], ok[2], codes, on_start, on_end)
        assert value.dtype == torch.uint8 and known.dtype == torch.uint8 and value.shape == (n,) and known.shape == (n,)
        assert np.array_equal(known.cpu().numpy(), want_known), op
        assert np.array_equal(value.cpu().numpy(), want_value), op
    return got


def _table(r, n, n_chrom=3, top=20_000):
    chrom = r.integers(0, n_chrom, n).astype(np.int32)
    start = r.integers(0, top, n).astype(np.int32)
    end = start + r.choice([1, 5, 40, 300, 2500], n).astype(np.int32)
    return chrom, start, end


def _ranges(r, k, n_chrom=3, top=20_000):
    """k ranges: mostly short, every 16th long."""
    out = []
    for i in range(k):
        lo = int(r.integers(0, top))
        out.append((int(r.integers(0, n_chrom)), lo, lo + int(r.integers(1, 60) if i % 16 else r.integers(2000, 9000))))
    return out


@pytest.mark.parametrize("k", [2, 3, 1024])
def test_against_the_reference_for_k_ranges(eng, k):
    r = np.random.default_rng(100 + k)
    chrom, start, end = _table(r, 3 * TILE + 17)
    ranges = _ranges(r, k)
    got = _check(eng, chrom, start, end, [_as_bounds(op, ranges) for op in OPS])
    for value, _known in got:       # (a check that matches nothing, or everything, would show little)
        assert 0 < int(value.sum()) < len(chrom)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 17])
def test_row_counts_around_the_wave_and_the_tile(eng, n):
    r = np.random.default_rng(n)
    chrom, start, end = _table(r, n, top=3000)
    ranges = _ranges(r, 9, top=3000)
    _check(eng, chrom, start, end, [_as_bounds(op, ranges) for op in OPS])


def test_columns_off_the_16_byte_grid_take_the_scalar_path(eng):
    r = np.random.default_rng(7)
    chrom, start, end = _table(r, 2 * TILE + 5, top=3000)
    ranges = _ranges(r, 12, top=3000)
    c, s, e = (_dev(x)[1:] for x in (chrom, start, end))     # views one int32 past an aligned allocation
    assert c.data_ptr() % 16 == 4
    for op in OPS:
        (value, known), = eng.range_set_any(c, s, e, [_as_bounds(op, ranges)])
        ones = np.ones(len(chrom) - 1, bool)
        want = ref.any_over_bounds(op, chrom[1:], start[1:], end[1:], ones, ones, ones, *_as_bounds(op, ranges)[1:])
        assert np.array_equal(value.cpu().numpy(), want[0]) and np.array_equal(known.cpu().numpy(), want[1])


def test_the_aggregate_does_not_leak_across_a_chromosome_boundary(eng):
    # chromosome 0 holds a huge range, chromosome 1 short ones only: a row of chromosome 1 whose search lands on the
    # first range of its segment must not see chromosome 0's maximum (nor, for CONTAINS, chromosome 2's minimum)
    ranges = [(0, 0, 1_000_000), (1, 500, 510), (1, 600, 610), (2, 0, 1)]
    chrom = np.array([1, 1, 1, 1, 0, 2, 1, 1], np.int32)
    start = np.array([100, 520, 0, 505, 100, 0, 400, 605], np.int32)
    end = np.array([200, 530, 100_000, 506, 200, 5, 700, 606], np.int32)
    got = _check(eng, chrom, start, end, [_as_bounds(op, ranges) for op in OPS])
    assert got[0][0].cpu().tolist() == [0, 0, 1, 1, 1, 1, 1, 1]     # intersects
    assert got[1][0].cpu().tolist() == [0, 0, 1, 0, 0, 1, 1, 0]     # contains
    assert got[2][0].cpu().tolist() == [0, 0, 0, 1, 1, 0, 0, 1]     # within


def test_a_match_only_the_aggregate_finds(eng):
    # one long range sorted well before the row's neighbours: the ranges beside the row's place in the order miss it
    short = [(0, 1000 + 100 * i, 1010 + 100 * i) for i in range(40)]
    ranges = [(0, 5, 100_000)] + short
    chrom = np.zeros(4, np.int32)
    start = np.array([3050, 3020, 3950, 200_000], np.int32)
    end = np.array([3060, 3080, 3960, 200_010], np.int32)
    got = _check(eng, chrom, start, end, [_as_bounds("intersects", ranges), _as_bounds("within", ranges),
                                         _as_bounds("intersects", short), _as_bounds("within", short)])
    assert got[0][0].cpu().tolist() == [1, 1, 1, 0] and got[1][0].cpu().tolist() == [1, 1, 1, 0]
    assert got[2][0].cpu().tolist() == [0, 0, 0, 0] and got[3][0].cpu().tolist() == [0, 0, 0, 0]
    # CONTAINS: the first range at or past the row's start is long; a later short one is the one the row contains
    ranges = [(0, 1000, 9000), (0, 1500, 1510), (0, 2000, 8000)]
    got = _check(eng, np.zeros(2, np.int32), np.array([900, 1200], np.int32), np.array([1600, 1505], np.int32),
                 [_as_bounds("contains", ranges)])
    assert got[0][0].cpu().tolist() == [1, 0]


def test_half_open_touching(eng):
    # a row that ends where the range starts, or starts where it ends, does not intersect it; a row that shares a
    # bound with the range is within it / contains it
    ranges = [(0, 100, 200), (0, 300, 400)]
    rows = [(50, 100), (200, 250), (200, 300), (99, 101), (199, 201), (100, 200), (100, 150), (150, 200), (300, 400),
            (100, 201), (99, 200)]
    chrom = np.zeros(len(rows), np.int32)
    start, end = (np.array(x, np.int32) for x in zip(*rows))
    got = _check(eng, chrom, start, end, [_as_bounds(op, ranges) for op in OPS])
    assert got[0][0].cpu().tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1]
    assert got[1][0].cpu().tolist() == [0, 0, 0, 0, 0, 1, 0, 0, 1, 1, 1]
    assert got[2][0].cpu().tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0]


def test_null_rows_are_three_valued(eng):
    r = np.random.default_rng(11)
    n = TILE + 77
    chrom, start, end = _table(r, n, n_chrom=4, top=3000)
    ranges = _ranges(r, 20, n_chrom=3, top=3000)        # (chromosome 3 is named by no range)
    valid = [r.random(n) >= 0.2 for _ in range(3)]
    got = _check(eng, chrom, start, end, [_as_bounds(op, ranges) for op in OPS], valid=valid)
    for value, known in got:
        known = known.cpu().numpy().astype(bool)
        assert (~known).any() and (known & ~(valid[0] & valid[1] & valid[2])).any()   # NULL answers, and settled ones
        assert not (value.cpu().numpy().astype(bool) & ~known).any()
    # a NULL start on a chromosome no range names: FALSE, not NULL
    off = (chrom == 3) & valid[0] & ~valid[1]
    assert off.any() and got[0][1].cpu().numpy()[off].all() and not got[0][0].cpu().numpy()[off].any()
    # one validity array only
    _check(eng, chrom, start, end, [_as_bounds("within", ranges)], valid=(None, None, valid[2]))


def test_codes_outside_every_range_and_outside_the_dictionary(eng):
    ranges = [(2, 0, 1000), (5, 0, 1000)]
    chrom = np.array([-1, 0, 1, 2, 3, 4, 5, 6, 2**31 - 1, -2**31], np.int32)
    start = np.full(len(chrom), 10, np.int32)
    end = np.full(len(chrom), 20, np.int32)
    got = _check(eng, chrom, start, end, [_as_bounds(op, ranges) for op in OPS])
    assert got[0][0].cpu().tolist() == [0, 0, 0, 1, 0, 0, 1, 0, 0, 0] and got[0][1].cpu().tolist() == [1] * len(chrom)


def test_bounds_at_the_ends_of_int64_and_rows_at_the_ends_of_int32(eng):
    lo, hi = -2**63, 2**63 - 1
    chrom = np.zeros(4, np.int32)
    start = np.array([-2**31, -2**31, 2**31 - 2, 0], np.int32)
    end = np.array([-2**31 + 1, 2**31 - 1, 2**31 - 1, 1], np.int32)
    _check(eng, chrom, start, end, [("intersects", [0, 0], [hi, lo], [lo, hi]), ("within", [0, 0], [lo, hi], [hi, lo]),
                                    ("contains", [0, 0], [hi, lo], [lo, hi])])


def test_bad_arguments_are_refused(eng):
    z = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    one = ("intersects", [0], [5], [1])
    with pytest.raises(ValueError):
        eng.range_set_any(z, z, z, [])
    with pytest.raises(ValueError):
        eng.range_set_any(z, z, z, [one] * 9)
    with pytest.raises(ValueError):
        eng.range_set_any(z, z, z, [("overlaps", [0], [5], [1])])
    with pytest.raises(ValueError):
        eng.range_set_any(z, z, z, [("within", list(range(1025)), list(range(1025)), list(range(1025)))])
    with pytest.raises(ValueError):
        eng.range_set_any(z, z.long(), z, [one])
    with pytest.raises(ValueError):
        eng.range_set_any(z, z, z[:3], [one])


@pytest.mark.parametrize("n_rows", [64, 0], ids=["rows", "no_rows"])
@pytest.mark.parametrize("kind", ["INNER", "CONTAINS"])
def test_the_call_drops_a_plan_the_context_keeps(eng, kind, n_rows):
    """The entry point's cells of the plan-lifetime table (include/giql_hip.h, THE LIFETIME OF A PLAN): it begins a
    call, so a plan kept in the context is dropped -- its fill answers GIQL_ERR_STATE and writes nothing -- whether the
    call then launches its kernel or returns at once because the table has no rows."""
    from giql_amd import _lib
    from giql_amd.engine import DeviceSide

    r = np.random.default_rng(3)
    a = DeviceSide.from_numpy(*_table(r, 300, top=3000))
    b = DeviceSide.from_numpy(*_table(r, 200, top=3000))
    plan, fill = (eng.inner_plan, eng.inner_fill) if kind == "INNER" else (eng.contain_plan, eng.contain_fill)
    n_pairs = plan(a, b, 3)
    assert n_pairs > 0
    outs = [torch.full((n_pairs + 8,), -7, dtype=torch.int32, device="cuda:0") for _ in range(2)]
    fill(*outs)                                      # the plan is there: its fill succeeds (and may be repeated)
    assert int((outs[0] >= 0).sum()) == n_pairs
    z = torch.zeros(n_rows, dtype=torch.int32, device="cuda:0")
    eng.range_set_any(z, z, z, [("intersects", [0, 0], [5, 9], [1, 7])])
    outs = [torch.full((n_pairs + 8,), -7, dtype=torch.int32, device="cuda:0") for _ in range(2)]
    with pytest.raises(_lib.GiqlHipError) as exc:
        fill(*outs)
    assert exc.value.code == _lib.GIQL_ERR_STATE and "without a successful" in str(exc.value)
    assert all(bool((o == -7).all()) for o in outs)


# ------------------------------------------------------------------------------------------------ execute()
def _arrow_table(case):
    import pyarrow as pa

    cols = case["columns"]
    return pa.table({"chrom": pa.array(cols["chrom"], pa.string()), "start": pa.array(cols["start"], pa.int32()),
                     "end": pa.array(cols["end"], pa.int32()), "score": pa.array(cols["score"], pa.int64())})


def _giql_tables(case):
    from giql_amd.table import Table

    return [Table("t", coordinate_system=case["encoding"][0], interval_type=case["encoding"][1])]


@pytest.mark.parametrize("k", range(len(GOLDEN["cases"])), ids=lambda k: GOLDEN["cases"][k]["name"].split(":")[0])
def test_execute_gives_every_golden_answer(eng, k):
    from giql_amd.execute import execute

    case = GOLDEN["cases"][k]
    ids = execute("SELECT * FROM t WHERE " + case["where"], {"t": _arrow_table(case)}, eng, giql_tables=_giql_tables(case),
                  return_indices=True, range_sets=True)
    assert ids.tolist() == case["expected"], case["name"]


def test_a_filter_that_mixes_a_set_a_folded_all_a_not_and_a_comparison(eng):
    import pyarrow as pa

    from giql_amd.execute import execute
    from giql_amd.transpile import build_plan

    r = np.random.default_rng(5)
    n = 2 * TILE + 31
    chrom = r.choice(["chr1", "chr2", "chr3"], n)
    start = r.integers(0, 5000, n).astype(np.int32)
    end = start + r.choice([1, 10, 100, 1500], n).astype(np.int32)
    score = r.integers(0, 100, n)
    name = np.array([f"row{i}" for i in range(n)])
    tbl = pa.table({"chrom": chrom, "start": start, "end": end, "score": score, "name": name})
    q = ("SELECT name, start AS s FROM t WHERE interval INTERSECTS ANY('chr1:1000-1200', 'chr1:[3000,3100]', 'chr2:50-4000', 'chr9:1-2') "
         "AND interval CONTAINS ALL('chr1:1100', 'chr1:1150') AND NOT interval WITHIN 'chr1:1000-2000' "
         "AND NOT interval INTERSECTS SOME('chr1:2400-2450', 'chr2:1-100000') AND score >= 10")
    plan = build_plan(q, None, range_sets=True)
    assert len(plan.range_sets) == 2 and len(plan.residuals) == 7
    c1 = chrom == "chr1"
    any_ = (c1 & (start < 1200) & (end > 1000)) | (c1 & (start < 3101) & (end > 3000)) | ((chrom == "chr2") & (start < 4000) & (end > 50))
    all_ = c1 & (start <= 1100) & (end >= 1151)
    within = c1 & (start >= 1000) & (end <= 2000)
    some = (c1 & (start < 2450) & (end > 2400)) | ((chrom == "chr2") & (start < 100000) & (end > 1))
    want = np.flatnonzero(any_ & all_ & ~within & ~some & (score >= 10))
    assert 0 < want.size < n
    assert execute(plan, {"t": tbl}, eng, return_indices=True).tolist() == want.tolist()
    out = execute(plan.to_string(), {"t": tbl}, eng)
    assert out.column_names == ["name", "s"]
    assert out.column("name").to_pylist() == name[want].tolist() and out.column("s").to_pylist() == start[want].tolist()


def test_a_pinned_table_is_uploaded_once(eng, monkeypatch):
    import pyarrow as pa

    import giql_amd
    from giql_amd import execute as ex_mod
    from giql_amd.engine import DeviceSide

    r = np.random.default_rng(9)
    n = ex_mod._CODES_CACHE_MIN_ROWS          # the smallest table whose codes and device copy are kept
    chrom = pa.array(r.choice(["chr1", "chr2", "chrX"], n))
    start = r.integers(0, 1_000_000, n).astype(np.int32)
    end = start + r.integers(1, 500, n).astype(np.int32)
    tbl = pa.table({"chrom": chrom, "start": start, "end": end})
    uploads = []
    real = DeviceSide.from_numpy.__func__
    monkeypatch.setattr(DeviceSide, "from_numpy", classmethod(lambda cls, *a, **k: (uploads.append(1), real(cls, *a, **k))[1]))
    q = "SELECT * FROM t WHERE interval INTERSECTS ANY('chr1:1000-5000', 'chrX:[700000,800000)', 'chr7:1-9')"
    want = np.flatnonzero(((chrom.to_numpy(zero_copy_only=False) == "chr1") & (start < 5000) & (end > 1000))
                          | ((chrom.to_numpy(zero_copy_only=False) == "chrX") & (start < 800000) & (end > 700000)))
    with giql_amd.pin(tbl) as pinned:
        for _ in range(2):
            ids = ex_mod.execute(q, {"t": pinned}, eng, return_indices=True, range_sets=True)
            assert ids.tolist() == want.tolist() and want.size
        assert len(uploads) == 1
        negated = ex_mod.execute(q.replace("WHERE", "WHERE NOT"), {"t": pinned}, eng, return_indices=True, range_sets=True)
        assert negated.size == n - want.size and len(uploads) == 1
