"""The vectorised reference of the one-table family (``tests/_one_table_ref.py``) against the row-by-row ones --
``ora.py_cluster`` / ``py_merge`` (the window SQL in plain Python), their C restatements, ``_merge_agg_ref.merge_agg``
and ``_string_agg_ref.merge_string_agg`` -- on 240 seeded tables of 1 to 400 rows.  No GPU.

A table is built in sorted order, one chromosome after the other, so that every step can be aimed: a row starts on its
predecessor's start, exactly on ``running MAX(end) + distance`` (the last start that still merges), one past it (the
first that does not), inside the running region, or far away; rows of length 0 are common.  Then the rows are shuffled.
Every property the construction aims at is counted over the tables and asserted to occur."""
import functools

import numpy as np
import pytest

import _merge_agg_ref as R
import _one_table_ref as V
import _string_agg_ref as S
from oracle import pyoracle as ora

N_TABLES = 240
DISTANCES = (0, 1, 30)
FIVE = ("COUNT", "SUM", "MIN", "MAX", "AVG")
TYPES = {"i32": np.int32, "i64": np.int64, "f32": np.float32, "f64": np.float64}


def build_table(seed):
    r = np.random.default_rng(9000 + seed)
    distance = DISTANCES[seed % 3]
    n = [1, 2, 3, 400][seed] if seed < 4 else int(1 + 399 * r.random() ** 3)
    n_chrom = int(r.integers(1, 5))
    per = np.bincount(r.integers(0, n_chrom, n), minlength=n_chrom)
    chrom, start, end, region, seen = [], [], [], [], {"equal": 0, "touch": 0, "past": 0, "zero": 0}
    g = -1
    for c in range(n_chrom):
        s_prev = run = None
        for _ in range(int(per[c])):
            step = r.choice(["equal", "touch", "past", "inside", "far"], p=[0.25, 0.15, 0.15, 0.3, 0.15])
            if s_prev is None:
                s, step = int(r.integers(-50, 50)), "first"
            elif step == "equal":
                s = s_prev
            elif step == "touch":
                s = run + distance
            elif step == "past":
                s = run + distance + 1
            elif step == "inside":
                s = int(r.integers(s_prev, run + 1))
            else:
                s = run + distance + int(r.integers(2, 200))
            ln = int(r.choice([0, 0, 1, 2, 7, 40]))
            if s_prev is None or s > run + distance:
                g += 1
            elif step in seen:
                seen[step] += 1
            seen["past"] += step == "past"
            seen["zero"] += ln == 0
            chrom.append(c), start.append(s), end.append(s + ln), region.append(g)
            s_prev, run = s, (s + ln if run is None else max(run, s + ln))
    order = r.permutation(n)
    chrom, start, end, region = (np.array(x, np.int64)[order] for x in (chrom, start, end, region))
    null_regions = r.choice(g + 1, max(1, (g + 1) // 6), replace=False)        # regions whose every value is NULL
    dead = np.isin(region, null_regions)
    cols = {}
    for name, dtype in TYPES.items():
        if np.dtype(dtype).kind == "i":
            vals = r.integers(-1_000_000, 1_000_000, n).astype(dtype)
        else:
            vals = (r.normal(0, 1000, n) * r.choice([1e-3, 1.0, 1e3], n)).astype(dtype)
            vals[r.random(n) < 0.04] = np.nan
        cols[name] = (vals, (r.random(n) >= 0.3) & ~dead)
    words = [None if dead[i] or r.random() < 0.3 else (b"" if r.random() < 0.1 else b"%d:" % i + bytes(r.integers(97, 123, int(r.integers(0, 6)), dtype=np.uint8)))
             for i in range(n)]
    seen.update(nan=int(sum(np.isnan(v[ok]).sum() for v, ok in cols.values() if v.dtype.kind == "f")),
                null_regions=len(null_regions), regions=g + 1)
    return chrom, start, end, n_chrom, distance, cols, words, seen


@functools.lru_cache(maxsize=None)
def table(seed):
    return build_table(seed)


def _py(col):
    vals, valid = col
    return [v.item() if ok else None for v, ok in zip(vals, valid)]


def _same(a, b) -> bool:
    return a == b or (isinstance(a, float) and isinstance(b, float) and a != a and b != b)


def test_the_tables_hold_what_the_construction_aims_at():
    seen = [table(k)[-1] for k in range(N_TABLES)]
    sizes = [len(table(k)[0]) for k in range(N_TABLES)]
    assert N_TABLES >= 200 and min(sizes) == 1 and max(sizes) == 400
    for d in DISTANCES:
        mine = [s for k, s in enumerate(seen) if DISTANCES[k % 3] == d]
        for what in ("equal", "touch", "past", "zero", "nan", "null_regions"):
            assert sum(s[what] for s in mine) > 50, (d, what)
    # the construction's own region count is the reference's: ``touch`` merged, ``past`` did not
    for k in range(N_TABLES):
        chrom, start, end, _nc, distance, _cols, _words, s = table(k)
        assert V.Layout(chrom, start, end, distance).m == s["regions"], k


@pytest.mark.parametrize("block", range(8))
def test_cluster_and_merge_equal_the_window_sql_in_plain_python(block):
    for k in range(block, N_TABLES, 8):
        chrom, start, end, _nc, distance, _cols, _words, _seen = table(k)
        side = ora.Side(chrom, start, end)
        lay = V.Layout(chrom, start, end, distance)
        assert np.array_equal(lay.cluster_ids(), ora.py_cluster(side, distance)), k
        assert np.array_equal(lay.cluster_ids(), ora.c_cluster(side, distance)), k
        rows = [tuple(int(x) for x in row) for row in zip(*lay.merge_rows())]
        assert rows == ora.py_merge(side, distance), k
        assert all(np.array_equal(a, b) for a, b in zip(lay.merge_rows(), ora.c_merge(side, distance))), k
        # (another distance than the one the table was aimed at)
        other = V.Layout(chrom, start, end, 7)
        assert np.array_equal(other.cluster_ids(), ora.c_cluster(side, 7)), k


@pytest.mark.parametrize("block", range(4))
def test_aggregates_equal_the_row_by_row_reference(block):
    for k in range(block, N_TABLES, 4):
        chrom, start, end, _nc, distance, cols, _words, _seen = table(k)
        lay = V.Layout(chrom, start, end, distance)
        aggs = [(f, c) for c in TYPES for f in FIVE]
        ref = R.merge_agg(chrom.tolist(), start.tolist(), end.tolist(), distance, {c: _py(cols[c]) for c in TYPES}, aggs)
        assert [row[:4] for row in ref] == [[int(x) for x in row] for row in zip(*lay.merge_rows())], k
        for j, (func, c) in enumerate(aggs):
            vals, valid = lay.aggregate(func, *cols[c])
            flt = cols[c][0].dtype.kind == "f"
            assert vals.dtype == (np.int64 if func == "COUNT" or (not flt and func != "AVG") else np.float64), (func, c)
            got = [v.item() if ok else None for v, ok in zip(vals, valid)]
            want = [row[4 + j] for row in ref]
            assert all(_same(a, b) for a, b in zip(got, want)) and len(got) == len(want), (k, func, c)
        # the error bound's scale
        xs = _py(cols["f64"])
        for g, (_p, members) in enumerate(R.regions(chrom.tolist(), start.tolist(), end.tolist(), distance)):
            assert lay.abs_sum(*cols["f64"])[g] == R.abs_sum([xs[i] for i in members]), (k, g)
            if g > 3:
                break


@pytest.mark.parametrize("block", range(4))
def test_string_agg_equals_the_row_by_row_reference(block):
    for k in range(block, N_TABLES, 4):
        chrom, start, end, _nc, distance, _cols, words, _seen = table(k)
        lay = V.Layout(chrom, start, end, distance)
        seps = [b",", b"", b"; "]
        ref = S.merge_string_agg(chrom.tolist(), start.tolist(), end.tolist(), distance, {"w": words}, [("w", s) for s in seps])
        for j, sep in enumerate(seps):
            assert lay.strings(words, sep) == [row[4 + j] for row in ref], (k, sep)
        off, data, ok = lay.string_agg(words, b",")
        assert all(off[g] == off[g + 1] for g in range(lay.m) if not ok[g])


def test_an_integer_sum_that_could_reach_2_63_is_refused():
    lay = V.Layout([0, 0], [0, 1], [5, 6])
    with pytest.raises(AssertionError, match="2\\^63"):
        lay.aggregate("SUM", np.array([2**62, 2**62], np.int64))
    assert lay.aggregate("SUM", np.array([2**62, 2**62 - 1], np.int64))[0].tolist() == [2**63 - 1]
