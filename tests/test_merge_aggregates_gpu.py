"""Aggregates beside MERGE on the GPU: ``HipEngine.merge_agg`` and ``execute(..., merge_aggregates=True)`` against
tests/_merge_agg_ref.py (exact arithmetic over the oracle's cluster ids) and the sqlite-minted rows of
tests/golden/merge_aggregates.json.

Exactness: counts, integer results and MIN / MAX compare with ``==``; AVG over an integer column too (|sum| < 2^53
here, so ``float(sum) / count`` is the only rounding).  A float SUM over k non-NULL values may differ from ``fsum``
by at most k * 2^-52 * sum|x_i| -- the standard bound (k - 1) * u * sum|x_i|, u = 2^-53, for ANY summation order in
binary64, doubled -- and a float AVG by that over k plus one ulp of the result (the division).  Derived, not
measured."""
import ctypes
import json
import math
import os

import numpy as np
import pytest

import _merge_agg_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "merge_aggregates.json")))
TILE = 256   # MAGG_TILE (giql_amd/csrc/merge_agg_kernels.hip.h): sorted positions per block
FIVE = ("COUNT", "SUM", "MIN", "MAX", "AVG")


@pytest.fixture(scope="module")
def eng():
    from giql_amd.engine import HipEngine

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    e = HipEngine(0)
    yield e
    e.close()


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _column(r, n, dtype, nulls=0.3):
    """(values, valid): seeded, about 30 % NULLs; integer sums stay far below 2^53."""
    if np.dtype(dtype).kind == "i":
        vals = r.integers(-1_000_000, 1_000_000, n).astype(dtype)
    else:
        vals = (r.normal(0, 1000, n) * r.choice([1e-3, 1.0, 1e3], n)).astype(dtype)
    return vals, (r.random(n) >= nulls)


def _py(col):
    vals, valid = col
    return [v.item() if ok else None for v, ok in zip(vals, valid)] if valid is not None else [v.item() for v in vals]


def _same(a, b) -> bool:
    return a == b or (isinstance(a, float) and isinstance(b, float) and a != a and b != b)


def run_and_check(eng, chrom, start, end, n_chrom, distance, cols, aggs, preds=None, holds=None):
    """``eng.merge_agg`` over the numpy table against the reference, region by region.  ``cols``: name -> (values,
    valid | None); ``aggs``: ``[(func, name)]``.  Returns the engine's result."""
    from giql_amd.engine import DeviceSide

    side = DeviceSide.from_numpy(chrom.astype(np.int32), start.astype(np.int32), end.astype(np.int32), device="cuda:0")
    dev = {k: (_dev(v), None if ok is None else _dev(ok.astype(np.uint8))) for k, (v, ok) in cols.items()}
    out = eng.merge_agg(side, n_chrom, distance, [(f,) + dev[c] for f, c in aggs], preds=preds)
    regions = R.regions(chrom.tolist(), start.tolist(), end.tolist(), distance, holds)
    py = {k: _py(c) for k, c in cols.items()}
    c, s, e, cnt = (t.cpu().tolist() for t in out[:4])
    assert len(out) == 4 + len(aggs)
    assert c == [p for p, _m in regions]
    assert s == [min(int(start[i]) for i in m) for _p, m in regions]
    assert e == [max(int(end[i]) for i in m) for _p, m in regions]
    assert cnt == [len(m) for _p, m in regions]
    for j, (func, name) in enumerate(aggs):
        vals, valid = (t.cpu().tolist() for t in out[4 + j])
        flt = cols[name][0].dtype.kind == "f"
        assert out[4 + j][0].dtype == (torch.int64 if func == "COUNT" or (not flt and func != "AVG") else torch.float64)
        for g, (_p, members) in enumerate(regions):
            xs = [py[name][i] for i in members]
            want = R.aggregate(func, xs)
            what = f"{func}({name}) region {g} of {len(members)} rows"
            assert valid[g] == (want is not None), what
            if want is None:
                continue
            k = sum(x is not None for x in xs)
            if flt and func in ("SUM", "AVG") and want == want and not math.isinf(want):
                bound = k * 2.0**-52 * R.abs_sum(xs)
                bound = bound if func == "SUM" else bound / k + math.ulp(want)
                assert abs(vals[g] - want) <= bound, (what, vals[g], want, bound)
            else:
                assert _same(vals[g], want), (what, vals[g], want)
    return out


def _random_table(r, n, n_part=5):
    chrom = r.integers(0, n_part, n)
    start = r.integers(0, max(20 * n // n_part, 50), n)
    return chrom, start, start + r.integers(1, 60, n)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1000, 5000])
def test_random_tables_every_function_over_every_type(eng, n):
    r = np.random.default_rng(100 + n)
    chrom, start, end = _random_table(r, n)
    for dtype in (np.int32, np.int64, np.float32, np.float64):
        cols = {"v": _column(r, n, dtype)}
        run_and_check(eng, chrom, start, end, 5, 0, cols, [(f, "v") for f in FIVE])
    run_and_check(eng, chrom, start, end, 5, 30, {"v": _column(r, n, np.float64)}, [("SUM", "v"), ("AVG", "v")])


def _built_regions(r, lengths, shuffle=True):
    """One partition whose merged regions have exactly ``lengths`` rows: inside a region every interval overlaps
    every other; regions lie 2000 apart.  Returns chrom, start, end and the region index per row."""
    start = np.concatenate([2000 * j + np.arange(L) % 900 for j, L in enumerate(lengths)])
    end = np.concatenate([np.full(L, 2000 * j + 1000) for j, L in enumerate(lengths)])
    region = np.concatenate([np.full(L, j) for j, L in enumerate(lengths)])
    order = r.permutation(len(start)) if shuffle else np.arange(len(start))
    return np.zeros(len(start), np.int64), start[order], end[order], region[order]


EDGE_AGGS = [("SUM", "f"), ("MIN", "f"), ("MAX", "f"), ("COUNT", "f"), ("AVG", "f"), ("SUM", "i"), ("MIN", "i"), ("AVG", "i")]


@pytest.mark.parametrize("lengths", [
    [64], [65], [256], [257], [2 * TILE + 1], [5000],                    # one region = all n rows
    [3, 64, 5], [3, 65, 5], [1, 256, 2], [7, 257, 1], [9, 2 * TILE + 1, 4],
    [300, 1, 300],                                                       # one row between two long regions
    [64, 64, 128, 256, 256, 1, 255, 512, 7],                             # boundaries on wave and tile edges
    [TILE - 1, 1, TILE, 64 * TILE, 1, 1, 3 * TILE + 7],                  # a region across more tiles than a fold step
], ids=lambda v: "-".join(map(str, v)))
def test_region_length_edges(eng, lengths):
    r = np.random.default_rng(7)
    chrom, start, end, _region = _built_regions(r, lengths)
    n = len(start)
    cols = {"f": _column(r, n, np.float64), "i": _column(r, n, np.int64)}
    out = run_and_check(eng, chrom, start, end, 1, 0, cols, EDGE_AGGS)
    assert out[3].cpu().tolist() == lengths


@pytest.mark.parametrize("null_regions", [(0,), (2,), (4,), (0, 2, 4)], ids=str)
def test_a_region_that_is_all_null(eng, null_regions):
    r = np.random.default_rng(8)
    chrom, start, end, region = _built_regions(r, [70, 300, 5, 260, 3])
    n = len(start)
    cols = {"f": _column(r, n, np.float64), "i": _column(r, n, np.int64)}
    for vals, valid in cols.values():
        valid[np.isin(region, null_regions)] = False
    out = run_and_check(eng, chrom, start, end, 1, 0, cols, EDGE_AGGS)
    assert [g for g, ok in enumerate(out[4][1].cpu().tolist()) if not ok] == list(null_regions)
    assert all(out[4 + 3][1].cpu().tolist())                             # COUNT is always valid ...
    assert [out[4 + 3][0].cpu().tolist()[g] for g in null_regions] == [0] * len(null_regions)   # ... and 0 there


def test_shared_and_separate_columns_and_eight_aggregates(eng):
    r = np.random.default_rng(9)
    chrom, start, end = _random_table(r, 3000)
    cols = {"a": _column(r, 3000, np.float64), "b": _column(r, 3000, np.int32), "c": (_column(r, 3000, np.float32)[0], None)}
    run_and_check(eng, chrom, start, end, 5, 0, cols, [("SUM", "a"), ("MAX", "a"), ("SUM", "b"), ("MIN", "c")])
    run_and_check(eng, chrom, start, end, 5, 0, cols, [("SUM", "a"), ("AVG", "a")])        # one kernel aggregate
    eight = [(f, c) for c in ("a", "b") for f in ("COUNT", "SUM", "MIN", "MAX")]
    run_and_check(eng, chrom, start, end, 5, 0, cols, eight)
    run_and_check(eng, chrom, start, end, 5, 0, cols, [(f, c) for f, c in eight[:6]] + [("AVG", "a"), ("AVG", "b")])


def test_zero_and_nine_aggregates_are_errors(eng):
    from giql_amd import _lib
    from giql_amd.engine import DeviceSide

    r = np.random.default_rng(10)
    chrom, start, end = _random_table(r, 100)
    side = DeviceSide.from_numpy(chrom.astype(np.int32), start.astype(np.int32), end.astype(np.int32), device="cuda:0")
    v = _dev(r.normal(size=100))
    for aggs in ([], [("SUM", v, None)] * 9):
        with pytest.raises(ValueError, match="1 to 8 aggregates"):
            eng.merge_agg(side, 5, 0, aggs)
    with pytest.raises(ValueError, match="aggregate function"):
        eng.merge_agg(side, 5, 0, [("MEDIAN", v, None)])
    with pytest.raises(ValueError, match="one value per row"):
        eng.merge_agg(side, 5, 0, [("SUM", v[:50].contiguous(), None)])
    # the C ABI says the same, and names the aggregate, before anything is launched
    out = torch.empty(100, dtype=torch.int64, device="cuda:0")
    c_aggs = (_lib.CAgg * 9)()
    for a in c_aggs:
        a.func, a.type, a.data, a.out = 1, _lib.T_F64, v.data_ptr(), out.data_ptr()
    m = ctypes.c_int64(-1)

    def call(aggs, k):
        return eng._L.giql_hip_merge_agg_dev(eng._h, side.c_struct(), 5, 0, None, 0, aggs, k, out.data_ptr(),
                                             out.data_ptr(), out.data_ptr(), None, 100, ctypes.byref(m), None)

    for k in (0, 9, -1):
        assert call(c_aggs, k) == _lib.GIQL_ERR_INVALID
        assert b"aggregates" in eng._L.giql_hip_last_error()
    for field, value, message in (("func", 4, b"aggregate 2: function 4"), ("type", _lib.T_U8, b"aggregate 2: column type"),
                                  ("data", None, b"aggregate 2: data or out is NULL"),
                                  ("out", None, b"aggregate 2: data or out is NULL")):
        keep = getattr(c_aggs[2], field)
        setattr(c_aggs[2], field, value)
        assert call(c_aggs, 3) == _lib.GIQL_ERR_INVALID
        assert message in eng._L.giql_hip_last_error()
        setattr(c_aggs[2], field, keep)


def test_an_empty_table(eng):
    from giql_amd.engine import DeviceSide

    z = np.zeros(0, np.int32)
    out = eng.merge_agg(DeviceSide.from_numpy(z, z, z, device="cuda:0"), 1, 0,
                        [("SUM", _dev(np.zeros(0)), None), ("COUNT", _dev(np.zeros(0, np.int32)), None)])
    assert [int(t.numel()) for t in out[:4]] == [0] * 4 and [int(v.numel()) for v, _ok in out[4:]] == [0, 0]


def test_predicate_regions_longer_than_a_wave_under_a_long_shadow(eng):
    # depth runs of 150 rows split the merge; row 0 reaches past everything, so every region ends while an earlier
    # one still reaches further (the regions are the predicate's, not the running maximum's)
    r = np.random.default_rng(11)
    n = 2000
    start = np.sort(r.choice(60_000, n, replace=False))
    end = start + r.integers(20, 400, n)
    end[0] = 70_000
    depth = np.repeat(r.permutation(n // 150 + 1), 150)[:n].astype(np.int64)
    order = r.permutation(n)
    start, end, depth = start[order], end[order], depth[order]
    d = _dev(depth)
    cols = {"f": _column(r, n, np.float64), "i": _column(r, n, np.int32)}
    out = run_and_check(eng, np.zeros(n, np.int64), start, end, 1, 0, cols,
                        [("SUM", "f"), ("AVG", "f"), ("MAX", "f"), ("SUM", "i"), ("MIN", "i"), ("COUNT", "i")],
                        preds=[(("a", d), "=", ("b", d))], holds=lambda i, j: depth[i] == depth[j])
    assert int(out[0].numel()) >= n // 150 and int(out[3].max()) >= 150


def test_a_genome_wider_than_the_32_bit_axis(eng):
    from giql_amd import _lib
    from giql_amd.engine import DeviceSide

    r = np.random.default_rng(12)
    n = 700
    chrom = r.integers(0, 2, n)
    start = np.where(r.random(n) < 0.5, r.integers(0, 40_000, n), 2_147_000_000 + r.integers(0, 40_000, n))
    end = start + r.integers(1, 600, n)
    # each chromosome spans [0, 2^31 - 1] exactly, as the "tight_over" layout of tests/test_axis_edges.py: 2^32 in all
    chrom[:4] = [0, 0, 1, 1]
    start[:4], end[:4] = [0, 2**31 - 101] * 2, [100, 2**31 - 1] * 2
    side = DeviceSide.from_numpy(chrom.astype(np.int32), start.astype(np.int32), end.astype(np.int32), device="cuda:0")
    assert sum(eng.chrom_spans(side, eng._empty_side(), 2)) == 2**32     # one call cannot hold both chromosomes
    with pytest.raises(_lib.GiqlHipError) as exc:
        eng._merge_agg_once(side, 2, 0, [("COUNT", _dev(np.zeros(n, np.int32)), None)])
    assert exc.value.code == _lib.GIQL_ERR_SPAN
    cols = {"f": _column(r, n, np.float64), "i": _column(r, n, np.int64)}
    run_and_check(eng, chrom, start, end, 2, 0, cols, EDGE_AGGS)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_nan_is_greater_than_every_number(eng, dtype):
    r = np.random.default_rng(13)
    chrom, start, end, region = _built_regions(r, [90, 300, 4])
    n = len(start)
    vals, valid = _column(r, n, dtype)
    vals[np.nonzero((region == 0) & valid)[0][[0, 5]]] = np.nan          # a NaN among numbers
    vals[region == 1] = np.nan                                           # only NaNs (and NULLs)
    out = run_and_check(eng, chrom, start, end, 1, 0, {"v": (vals, valid)}, [(f, "v") for f in FIVE])
    _cnt, total, lo, hi, _avg = (o[0].cpu().tolist() for o in out[4:])
    assert math.isnan(total[0]) and math.isnan(hi[0]) and not math.isnan(lo[0])
    assert math.isnan(lo[1]) and math.isnan(hi[1]) and not math.isnan(hi[2])


def test_the_same_float_sum_twice_is_bitwise_equal(eng):
    from giql_amd.engine import DeviceSide

    r = np.random.default_rng(14)
    chrom, start, end = _random_table(r, 5000)
    side = DeviceSide.from_numpy(chrom.astype(np.int32), start.astype(np.int32), end.astype(np.int32), device="cuda:0")
    vals, valid = _column(r, 5000, np.float64)
    v, ok = _dev(vals), _dev(valid.astype(np.uint8))
    first = eng.merge_agg(side, 5, 40, [("SUM", v, ok)])[4]
    again = eng.merge_agg(side, 5, 40, [("SUM", v, ok)])[4]
    assert torch.equal(first[0].view(torch.int64), again[0].view(torch.int64)) and torch.equal(first[1], again[1])


# ---------------------------------------------------------------------------------------------- execute()
def _golden_table(pa):
    rows = GOLDEN["rows"]
    types = [pa.string(), pa.int32(), pa.int32(), pa.string(), pa.float64(), pa.int32()]
    return pa.table({c: pa.array([r[k] for r in rows], type=t) for k, (c, t) in enumerate(zip(GOLDEN["columns"], types))})


def _sig(v):
    return float(f"{v:.12g}") if isinstance(v, float) else v


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=lambda c: c["name"])
def test_execute_returns_the_sqlite_minted_rows(eng, case):
    # (the stranded case: partitions of (chrom, strand), re-sorted by (chrom, start) with the aggregates carried along)
    pa = pytest.importorskip("pyarrow")
    from giql_amd.execute import execute

    args = "interval" + (f", {case['distance']}" if case["distance"] else "") + (", stranded := true" if case["stranded"] else "")
    keys = ["chrom"] + (["strand"] if case["stranded"] else []) + ["start", "end"]
    k = len(keys)
    for column, first in (("score", k + 1), ("weight", k + 6)):
        names = [f"{f}_{column}" for f in ("count", "sum", "avg", "min", "max")]
        select = ", ".join(f"{n.split('_')[0].upper()}({column}) AS {n}" for n in names)
        out = execute(f"SELECT MERGE({args}), COUNT(*) AS n, {select} FROM features", {"features": _golden_table(pa)},
                      eng, giql_tables=["features"], merge_aggregates=True)
        assert out.column_names == keys + ["n"] + names
        flt = column == "score"
        assert [str(out.schema.field(n).type) for n in ["n"] + names] == \
            ["int64", "int64", "double" if flt else "int64", "double", "double" if flt else "int32", "double" if flt else "int32"]
        got = [[_sig(v) for v in row] for row in zip(*(out.column(c).to_pylist() for c in out.column_names))]
        want = [[_sig(v) for v in row[:k + 1] + row[first:first + 5]] for row in case["merged"]]
        assert sorted(got, key=lambda x: (x[0], x[k - 2])) == sorted(want, key=lambda x: (x[0], x[k - 2]))
        assert [(x[0], x[k - 2]) for x in got] == sorted((x[0], x[k - 2]) for x in got)     # ORDER BY chrom, start


def test_execute_the_documented_recipes(eng):
    pa = pytest.importorskip("pyarrow")
    from giql_amd.execute import execute

    rows = GOLDEN["rows"]
    part = [r[0] for r in rows]
    columns = {"score": [r[4] for r in rows]}
    for query, distance, aggs in (
            ("SELECT MERGE(interval), AVG(score) AS avg_score FROM features", 0, [("AVG", "score")]),
            ("SELECT MERGE(interval), COUNT(*) AS feature_count, AVG(score) AS avg_score, MAX(score) AS max_score, "
             "SUM(score) AS total_score FROM features", 0, [("AVG", "score"), ("MAX", "score"), ("SUM", "score")]),
            ("SELECT MERGE(interval, 1000), COUNT(*) AS n, MAX(score) AS hi FROM features", 1000, [("MAX", "score")])):
        out = execute(query, {"features": _golden_table(pa)}, eng, giql_tables=["features"], merge_aggregates=True)
        ref = R.merge_agg(part, [r[1] for r in rows], [r[2] for r in rows], distance, columns, aggs)
        has_count = "COUNT(*)" in query
        want = [[_sig(v) for v in r[:3] + ([r[3]] if has_count else []) + r[4:]] for r in ref]
        got = [[_sig(v) for v in row] for row in zip(*(out.column(c).to_pylist() for c in out.column_names))]
        assert got == want, query
    with pytest.raises(ValueError, match="return_indices"):
        execute("SELECT MERGE(interval), AVG(score) AS a FROM features", {"features": _golden_table(pa)}, eng,
                giql_tables=["features"], merge_aggregates=True, return_indices=True)
    with pytest.raises(ValueError, match="column 'strand'"):
        execute("SELECT MERGE(interval), MAX(strand) AS a FROM features", {"features": _golden_table(pa)}, eng,
                giql_tables=["features"], merge_aggregates=True)
    flags = _golden_table(pa).append_column("flag", pa.array([True] * len(rows)))
    with pytest.raises(ValueError, match="column 'flag'"):
        execute("SELECT MERGE(interval), MAX(flag) AS a FROM features", {"features": flags}, eng,
                giql_tables=["features"], merge_aggregates=True)


def test_execute_behind_a_where_filter_takes_the_values_by_the_kept_rows(eng):
    pa = pytest.importorskip("pyarrow")
    from giql_amd.execute import execute

    r = np.random.default_rng(15)
    n = 3000
    chrom, start, end = _random_table(r, n, 3)
    depth = r.integers(0, 4, n)
    (score, score_ok), (weight, weight_ok) = _column(r, n, np.float32), _column(r, n, np.int64)
    tbl = pa.table({"chrom": pa.array([f"chr{c + 1}" for c in chrom]), "start": pa.array(start, pa.int32()),
                    "end": pa.array(end, pa.int32()), "depth": pa.array(depth),
                    "score": pa.array(score, mask=~score_ok), "weight": pa.array(weight, mask=~weight_ok)})
    out = execute("SELECT MERGE(interval, 10), SUM(weight) AS w, COUNT(*) AS n, MIN(score) AS lo, AVG(weight) AS aw, "
                  "COUNT(score) AS k FROM t WHERE depth < 2", {"t": tbl}, eng, giql_tables=["t"], merge_aggregates=True)
    keep = np.nonzero(depth < 2)[0]
    assert 0 < len(keep) < n
    columns = {"score": [_py((score, score_ok))[i] for i in keep], "weight": [_py((weight, weight_ok))[i] for i in keep]}
    ref = R.merge_agg([f"chr{c + 1}" for c in chrom[keep]], start[keep].tolist(), end[keep].tolist(), 10, columns,
                      [("SUM", "weight"), ("MIN", "score"), ("AVG", "weight"), ("COUNT", "score")])
    assert out.column_names == ["chrom", "start", "end", "w", "n", "lo", "aw", "k"]
    assert str(out.schema.field("lo").type) == "float" and str(out.schema.field("w").type) == "int64"
    got = list(zip(*(out.column(c).to_pylist() for c in out.column_names)))
    assert got == [(x[0], x[1], x[2], x[4], x[3], x[5], x[6], x[7]) for x in ref]
