"""CLUSTER, MERGE and MERGE's aggregates (numeric and STRING_AGG) under every form of their sort -- needs a GPU
(but for the check of the cases themselves).

Every one-table operator goes through ``cluster_front`` (``giql_amd/csrc/giql_hip.hip``): the span pass, linearize,
``run_sort_onesweep(sort_by_start)`` carrying (key, end[, row id]), the prefix maximum of the end keys, the head flags and
their scan; then ``k_cluster_ids``, the merge kernels, ``k_magg_tiles`` / ``k_magg_fold`` and the STRING_AGG kernels read
the sorted order.  The answers lean on that sort more than a join's: STRING_AGG's bytes are defined as "start, then
input row" -- the sort must be stable in every form -- and a float SUM repeats bit for bit only if the sorted order does.
Truth is ``tests/_one_table_ref.py`` (``tests/test_one_table_ref.py`` holds it to the row-by-row references without a
GPU); the ``predicate :=`` calls keep the row-by-row references.

The sort forms.  ``run_sort_onesweep`` asks ``plan_sort`` (``sort_plan.h``) with the context's ``sort_tuning``.  Of the
switches of DESIGN.md section 6b this path honours GIQL_HIP_LOCAL_MIN_ROWS, GIQL_HIP_LOCAL_BITS, GIQL_HIP_NO_LOCAL_SORT,
GIQL_HIP_OS_ORDER, GIQL_HIP_OS_VARIANT (which also turns the three-stage form off), GIQL_HIP_OS_HELP_AFTER and, at the
call's read-back (``cluster_status`` -> ``read_meta``), GIQL_HIP_INJECT_TIMEOUT -- each has a context in the ``FORMS`` of
``tests/test_disjoin_paths.py``, imported here.  GIQL_HIP_LOCAL_MIN / MAX_BUCKET_ROWS and GIQL_HIP_NO_NARROW_BUCKETS act
through the density of the context's previous call (``guess.last_span``), which this family reads and never sets (its
calls end in ``collect_spans`` and report ``stats.span``; none calls ``note_span``): the ``one_table`` walks of
``tests/test_context_transitions.py`` run the family on such contexts.  GIQL_HIP_SORT=classic, NO_UNIFORM, NO_SPAN_HIST,
NO_COARSE_B, COARSE_MAX_GROUP_ROWS and NO_FUSE_COUNT are not read on this path and get no context.

What is compared.  Cluster ids, region rows, counts, integer results, MIN / MAX, validity and STRING_AGG bytes: exactly.
A float SUM over k non-NULL values against ``math.fsum`` within k * 2^-52 * sum|x_i|, an AVG within that over k plus one
ulp (the bound of ``tests/test_merge_aggregates_gpu.py``, derived there).  And across forms: the sort carries row ids
and is stable, so the sorted order -- and with it the kernels' fixed reduction tree -- is the same in every form: every
aggregate output of every form equals the ``default`` form's bit for bit, as do two calls within a form.
"""
import functools

import numpy as np
import pytest

import _merge_agg_ref as R
import _one_table_ref as V
from oracle import pyoracle as ora
from test_disjoin_paths import FORMS, LOCAL, OS_TILE, TOP, _assert_form, _engine

torch = pytest.importorskip("torch")

gpu = pytest.mark.gpu        # (the cases are checked without one: test_sort_cases_are_what_they_claim)

DEV = "cuda:0"
BS_CAP = 4096            # rows of one bucket the LDS sort holds (bucket_sort.hip.h); more: bucket_sort_big
MAGG_TILE = 256          # sorted positions per block of k_magg_tiles; k_magg_fold takes 64 tiles a step
FOLD_STEP = 64 * MAGG_TILE
DISTANCE = 25            # the non-zero distance of every case
PRED_MAX_ROWS = 5000     # the predicate calls keep the row-by-row reference
# the five functions over the four types, eight aggregates a call; the third call repeats the float SUM / AVG of the
# first two (two calls within a form: the same bits)
AGG_CALLS = (
    [("SUM", "f64"), ("MIN", "f64"), ("MAX", "f64"), ("COUNT", "f64"), ("AVG", "f64"), ("SUM", "i64"), ("MIN", "i64"), ("MAX", "i64")],
    [("SUM", "f32"), ("MIN", "f32"), ("MAX", "f32"), ("COUNT", "f32"), ("AVG", "f32"), ("COUNT", "i64"), ("AVG", "i64"), ("SUM", "i32")],
    [("MIN", "i32"), ("MAX", "i32"), ("COUNT", "i32"), ("AVG", "i32"), ("SUM", "f64"), ("AVG", "f64"), ("SUM", "f32"), ("AVG", "f32")],
)
AGG_DISTANCE = (0, 0, DISTANCE)
TYPES = {"i32": np.int32, "i64": np.int64, "f32": np.float32, "f64": np.float64}
SEPARATORS = (b",", b" | ")


# ---------------------------------------------------------------- the cases (seeded; checked on the CPU below)
def _table(r, n, span, max_len, n_chrom=1):
    c = r.integers(0, n_chrom, n)
    s = r.integers(0, span, n)
    ln = r.integers(1, max_len, n)
    ln[r.random(n) < 0.03] = 0
    s[0], c[0] = 0, 0                       # (one chromosome: the sort key of a row is its start)
    return c.astype(np.int64), s.astype(np.int64), (s + ln).astype(np.int64)


def _regions(lengths, r):
    """One chromosome whose merged regions at distance 0 and at DISTANCE have exactly ``lengths`` rows: inside a region
    every row overlaps every other, starts repeat every 900 rows, regions lie 2000 apart."""
    start = np.concatenate([2000 * j + np.arange(L) % 900 for j, L in enumerate(lengths)])
    end = np.concatenate([np.full(L, 2000 * j + 1000) for j, L in enumerate(lengths)])
    order = r.permutation(len(start))
    return np.zeros(len(start), np.int64), start[order].astype(np.int64), end[order].astype(np.int64)


def _columns(r, n):
    cols = {}
    for name, dtype in TYPES.items():
        if np.dtype(dtype).kind == "i":
            vals = r.integers(-1_000_000, 1_000_000, n).astype(dtype)
        else:
            vals = (r.normal(0, 1000, n) * r.choice([1e-3, 1.0, 1e3], n)).astype(dtype)
        cols[name] = (vals, r.random(n) >= 0.3)
    letters = r.integers(97, 123, (n, 5), dtype=np.uint8)
    null = r.random(n) < 0.2
    words = [None if null[i] else (b"%d:" % i + bytes(letters[i, :i % 6])) for i in range(n)]      # every name carries its row
    return cols, words


class Case:
    def __init__(self, cid, table, n_chrom, seed):
        self.id, self.n_chrom = cid, n_chrom
        self.chrom, self.start, self.end = table
        self.n = len(self.start)
        self.cols, self.words = _columns(np.random.default_rng(seed), self.n)
        self.depth = (self.start // 64) % 3        # rows of one start share it: a predicate region's first start is its own

    @functools.lru_cache(maxsize=None)
    def layout(self, distance):
        return V.Layout(self.chrom, self.start, self.end, distance)

    @functools.lru_cache(maxsize=None)
    def aggregate(self, distance, func, col):
        return self.layout(distance).aggregate(func, *self.cols[col])

    @functools.lru_cache(maxsize=None)
    def bound(self, distance, func, col):
        """The float SUM / AVG tolerance per region, and where it applies (a finite expected value)."""
        lay = self.layout(distance)
        k = lay.non_null(self.cols[col][1])
        want, _ok = self.aggregate(distance, func, col)
        b = k * 2.0**-52 * lay.abs_sum(*self.cols[col])
        if func == "AVG":
            b = b / np.maximum(k, 1) + np.spacing(np.abs(np.where(np.isfinite(want), want, 0.0)))
        return b, np.isfinite(want)

    @functools.lru_cache(maxsize=None)
    def strings(self, distance, sep):
        return self.layout(distance).string_agg(self.words, sep)

    def holds(self, i, j):
        return self.depth[i] == self.depth[j]

    @functools.lru_cache(maxsize=None)
    def pred_expected(self, distance):
        """Row by row: (cluster ids, rows of ``_merge_agg_ref.merge_agg`` with SUM / AVG / MAX of f64 and SUM / MIN /
        COUNT of i32, per region the float bound's k and sum|x|)."""
        part, start, end = self.chrom.tolist(), self.start.tolist(), self.end.tolist()
        ids = ora.py_cluster_predicate(part, start, end, distance, self.holds)
        py = {c: [v.item() if ok else None for v, ok in zip(*self.cols[c])] for c in ("f64", "i32")}
        rows = R.merge_agg(part, start, end, distance, py, PRED_AGGS, self.holds)
        scale = [(sum(py["f64"][i] is not None for i in m), R.abs_sum([py["f64"][i] for i in m]))
                 for _p, m in R.regions(part, start, end, distance, self.holds)]
        return ids, rows, scale


PRED_AGGS = [("SUM", "f64"), ("AVG", "f64"), ("MAX", "f64"), ("SUM", "i32"), ("MIN", "i32"), ("COUNT", "i32")]


@functools.lru_cache(maxsize=None)
def cases():
    r = np.random.default_rng(5150)
    out = {}

    def add(cid, table, n_chrom=1):
        out[cid] = Case(cid, table, n_chrom, 6000 + len(out))

    # around one and two onesweep tiles, and a look-back across five
    for n in (OS_TILE - 1, OS_TILE, OS_TILE + 1, 2 * OS_TILE + 1, 40_000):
        add(f"rows-{n}", _table(r, n, 150 * n, 400, n_chrom=2), 2)
    # one row alone in its bucket (at every bucket width) between empty buckets and crowded ones
    c, s, e = _table(r, 3_000, 60_000, 300)
    add("empty-and-one-row-buckets", (np.append(c, 0), np.append(s, 65_536 + 5), np.append(e, 3 * 65_536 + 7)))
    # keys 0 and 0xFFFFFFFE: chromosome 0 over [0, 2^31 - 1], chromosome 1 over [1, 2^31 - 1]
    hi = 2**31 - 1
    c, s, e = _table(r, 3_000, 50_000, 300, 2)
    s, e = s + 1, e + 1
    far = r.random(3_000) < 0.5
    s, e = np.where(far, hi - 60_000 + s, s), np.where(far, hi - 60_000 + e, e)
    c[:5], s[:5], e[:5] = [0, 0, 1, 1, 1], [0, hi - 9, 1, hi - 30, hi], [7, hi, 12, hi, hi]
    add("both-ends-of-the-axis", (c, s, e), 2)
    # equal starts in every bucket: 20,000 rows on 200 starts, two starts to a region, ends that differ
    j = r.integers(0, 200, 20_000)
    s = (j // 2) * 40_000 + (j % 2) * 1_000
    add("20000-rows-sharing-200-starts", (np.zeros(20_000, np.int64), s, s + r.integers(1, 3_000, 20_000)))
    # 9,000 rows inside one 8,192-key range (one bucket at every width, more than BS_CAP rows) beside ordinary buckets
    c, s, e = _table(r, 3_000, 400_000, 300)
    hs = 2 * 65_536 + r.integers(0, 8_192, 9_000)
    add("hot-bucket-above-bs-cap", (np.append(c, np.zeros(9_000, np.int64)), np.append(s, hs),
                                    np.append(e, hs + r.integers(0, 3, 9_000))))
    # regions of more than 64 aggregate tiles behind a sort of six onesweep tiles
    add("long-regions-across-fold-steps", _regions([1] * 3_000 + [20_500] + [1] * 5_000 + [17_000] + [1] * 100, r))
    return out


def test_sort_cases_are_what_they_claim():
    cs = cases()
    assert OS_TILE == 8192 and {f"rows-{n}" for n in (8191, 8192, 8193, 16385, 40000)} <= set(cs)
    for case in cs.values():
        assert case.n_chrom > 1 or (case.start.min() == 0 and case.chrom.max() == 0), case.id    # key == start
        for d in (0, DISTANCE):
            assert case.layout(d).m > 1, case.id
    case = cs["rows-40000"]
    assert 4 < case.layout(0).count.max() < MAGG_TILE and (case.layout(0).count == 1).sum() > 1000
    assert case.layout(DISTANCE).m < case.layout(0).m
    s = cs["empty-and-one-row-buckets"].start
    assert len(s) <= PRED_MAX_ROWS
    for w in (13, 14, 15, 16):
        per = np.bincount(s >> w, minlength=(4 << 16) >> w)
        assert per[(65_536 + 5) >> w] == 1 and (per == 0).any() and per.max() > 100, w
    case = cs["both-ends-of-the-axis"]
    c, s, e = case.chrom, case.start, case.end
    assert case.n <= PRED_MAX_ROWS
    assert sum(int(e[c == k].max() - s[c == k].min() + 1) for k in (0, 1)) == TOP      # the span: 2^32 - 1
    assert s[c == 0].min() == 0 and s[c == 1].max() == e[c == 1].max() == 2**31 - 1     # start keys 0 and 0xFFFFFFFE
    case = cs["20000-rows-sharing-200-starts"]
    assert len(np.unique(case.start)) == 200 and case.layout(0).m == 100
    starts, per_start = np.unique(case.start, return_counts=True)
    assert per_start.min() > 32 and all(per_start[starts >> 13 == b].max() > 32 for b in np.unique(starts >> 13))
    assert len(np.unique(np.stack([case.start, case.end], 1), axis=0)) > 15_000          # ends that differ
    off, data, ok = case.strings(0, b",")
    for g in (0, 57, 99):      # a region's names: ascending rows of its first start, then of its second -- not ascending
        ids = [int(t.split(b":")[0]) for t in data[off[g]:off[g + 1]].split(b",")]
        cut = [k for k in range(1, len(ids)) if ids[k] < ids[k - 1]]
        assert len(cut) == 1 and ids[:cut[0]] == sorted(ids[:cut[0]]) and ids[cut[0]:] == sorted(ids[cut[0]:]), g
    case = cs["hot-bucket-above-bs-cap"]
    hot = (case.start >= 2 * 65_536) & (case.start < 2 * 65_536 + 8_192)
    assert hot.sum() >= 9_000 > BS_CAP and len(np.unique(case.start[hot])) < 8_192
    assert all(len(np.unique(case.start[hot] >> w)) == 1 for w in (13, 14, 15, 16))
    assert np.bincount(case.start[~hot] >> 13).max() < BS_CAP
    case = cs["long-regions-across-fold-steps"]
    lay = case.layout(0)
    assert case.n > 5 * OS_TILE and np.array_equal(lay.count, case.layout(DISTANCE).count)
    long_ones = np.nonzero(lay.count > FOLD_STEP)[0]
    assert len(long_ones) == 2 and (lay.count == 1).sum() == 8_100
    for g in long_ones:        # each straddles two onesweep tile boundaries and more than 64 aggregate tiles
        a, b = int(lay.heads[g]), int(lay.heads[g] + lay.count[g])
        assert b // OS_TILE - a // OS_TILE >= 2 and a % OS_TILE and b % OS_TILE and b // MAGG_TILE - a // MAGG_TILE > 64
        assert len(np.unique(case.start[lay.order[a:b]])) == 900       # ties inside it


# ---------------------------------------------------------------- device side
def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@functools.lru_cache(maxsize=None)
def resident(cid):
    """The case's table and columns on the device: ``(side, {column: (values, valid)}, (offsets, data, valid), depth)``."""
    from giql_amd.engine import DeviceSide

    case = cases()[cid]
    side = DeviceSide.from_numpy(case.chrom.astype(np.int32), case.start.astype(np.int32), case.end.astype(np.int32), device=DEV)
    cols = {k: (_t(v), _t(ok.astype(np.uint8))) for k, (v, ok) in case.cols.items()}
    lens = np.array([0 if w is None else len(w) for w in case.words], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    data = np.frombuffer(b"".join(w or b"" for w in case.words), np.uint8).copy()
    names = (_t(off), _t(data), _t(np.array([w is not None for w in case.words], np.uint8)))
    return side, cols, names, _t(case.depth)


def _rows_equal(got, lay, what):
    want = lay.merge_rows()
    for g, w, name in zip(got[:4], want, ("chrom", "start", "end", "count")):
        g = g.cpu().numpy()
        assert g.shape == w.shape and np.array_equal(g, w), (what, name)


def _agg_equal(case, distance, func, col, got, what):
    vals, valid = (t.cpu().numpy() for t in got)
    want, ok = case.aggregate(distance, func, col)
    flt = case.cols[col][0].dtype.kind == "f"
    assert vals.dtype == want.dtype and np.array_equal(valid.astype(bool), ok), (what, "validity")
    if flt and func in ("SUM", "AVG"):
        bound, finite = case.bound(distance, func, col)
        worst = float(np.max(np.abs(vals - want)[finite] / np.maximum(bound[finite], 5e-324), initial=0.0))
        assert np.all(np.abs(vals - want)[finite] <= bound[finite]), (what, "worst error / bound", worst)
        assert np.array_equal(np.isnan(vals), np.isnan(want)), what
    else:
        assert np.array_equal(vals, want, equal_nan=flt), what


def _bits(out):
    """Every aggregate output of a merge_agg result as integers: float64 by its bit pattern."""
    return [t.view(torch.int64).cpu() if t.dtype == torch.float64 else t.cpu() for pair in out[4:] for t in pair]


def _agg_call(e, cid, k):
    side, cols, _names, _depth = resident(cid)
    return e.merge_agg(side, cases()[cid].n_chrom, AGG_DISTANCE[k], [(f,) + cols[c] for f, c in AGG_CALLS[k]])


def _str_call(e, cid):
    side, cols, names, _depth = resident(cid)
    entries = [("SUM",) + cols["f64"]] + [("STRING_AGG",) + names + (sep,) for sep in SEPARATORS]
    return e.merge_agg(side, cases()[cid].n_chrom, DISTANCE, entries)


DEFAULT_BITS = {}        # case -> the default form's aggregate outputs, computed once in the session


def default_bits(cid):
    if cid not in DEFAULT_BITS:
        e = _engine(FORMS["default"][0])
        try:
            DEFAULT_BITS[cid] = [_bits(_agg_call(e, cid, k)) for k in range(len(AGG_CALLS))] + [_bits(_str_call(e, cid)[:5])]
        finally:
            e.close()
    return DEFAULT_BITS[cid]


def _same_bits(got, want, what):
    assert len(got) == len(want) and all(g.shape == w.shape and torch.equal(g, w) for g, w in zip(got, want)), what


@pytest.fixture(scope="module", params=list(FORMS))
def form_eng(request):
    e = _engine(FORMS[request.param][0])
    e.form = request.param
    yield e
    e.close()


@gpu
@pytest.mark.parametrize("cid", list(cases()))
def test_family_under_every_sort_form(form_eng, cid):
    e, case = form_eng, cases()[cid]
    side, cols, names, depth = resident(cid)
    nch, what = case.n_chrom, (e.form, cid)
    for d in (0, DISTANCE):
        lay = case.layout(d)
        ids = e.cluster(side, nch, d).cpu().numpy()
        _assert_form(e)
        assert np.array_equal(ids, lay.cluster_ids()), (what, "cluster", d)
        got = e.merge(side, nch, d)
        _assert_form(e)
        _rows_equal(got, lay, (what, "merge", d))
        if cid == "both-ends-of-the-axis":
            assert e.stats()["span"] == TOP
    for k, aggs in enumerate(AGG_CALLS):
        out = _agg_call(e, cid, k)
        _assert_form(e)
        _rows_equal(out, case.layout(AGG_DISTANCE[k]), (what, "merge_agg", k))
        for (func, col), got in zip(aggs, out[4:]):
            _agg_equal(case, AGG_DISTANCE[k], func, col, got, (what, func, col))
        _same_bits(_bits(out), default_bits(cid)[k], (what, "merge_agg", k, "the default form's bits"))
    _same_bits(_bits(_agg_call(e, cid, 0)), default_bits(cid)[0], (what, "the same call twice"))      # within a form
    out = _str_call(e, cid)
    e.merge(side, nch, 0)        # (the string fill reports no sort: the form is read from a plain MERGE right after)
    _assert_form(e)
    _rows_equal(out, case.layout(DISTANCE), (what, "merge_agg with STRING_AGG"))
    _agg_equal(case, DISTANCE, "SUM", "f64", out[4], (what, "SUM beside STRING_AGG"))
    _same_bits(_bits(out[:5]), default_bits(cid)[3], (what, "SUM beside STRING_AGG", "the default form's bits"))
    _same_bits(_bits(out[:5])[:1], default_bits(cid)[2][8:9], (what, "SUM beside STRING_AGG equals the numeric call's"))
    for sep, (o, data, ok) in zip(SEPARATORS, out[5:]):
        w_off, w_data, w_ok = case.strings(DISTANCE, sep)
        assert np.array_equal(ok.cpu().numpy().astype(bool), w_ok), (what, sep, "validity")
        assert np.array_equal(o.cpu().numpy(), w_off), (what, sep, "offsets")
        assert data.cpu().numpy().tobytes() == w_data, (what, sep, "bytes")
    if case.n <= PRED_MAX_ROWS:
        _predicate_calls(e, case, side, cols, depth, what)


def _predicate_calls(e, case, side, cols, depth, what):
    preds = [(("a", depth), "=", ("b", depth))]
    for d in (0, DISTANCE):
        ids, rows, scale = case.pred_expected(d)
        assert np.array_equal(e.cluster(side, case.n_chrom, d, preds=preds).cpu().numpy(), ids), (what, "cluster_pred", d)
        _assert_form(e)
        got = [t.cpu().tolist() for t in e.merge(side, case.n_chrom, d, preds=preds)]
        _assert_form(e)
        assert [list(x) for x in zip(*got)] == [row[:4] for row in rows], (what, "merge_pred", d)
        out = e.merge_agg(side, case.n_chrom, d, [(f,) + cols[c] for f, c in PRED_AGGS], preds=preds)
        _assert_form(e)
        assert [list(x) for x in zip(*(t.cpu().tolist() for t in out[:4]))] == [row[:4] for row in rows], (what, "merge_agg pred", d)
        for j, (func, col) in enumerate(PRED_AGGS):
            vals, valid = (t.cpu().tolist() for t in out[4 + j])
            for g, row in enumerate(rows):
                want = row[4 + j]
                assert valid[g] == (want is not None), (what, func, col, g)
                if want is None:
                    continue
                if col == "f64" and func in ("SUM", "AVG"):
                    k, scale_g = scale[g]
                    bound = k * 2.0**-52 * scale_g
                    bound = bound if func == "SUM" else bound / k + np.spacing(abs(want))
                    assert abs(vals[g] - want) <= bound, (what, func, g, vals[g], want, bound)
                else:
                    assert vals[g] == want, (what, func, col, g, vals[g], want)
    assert len(case.pred_expected(0)[1]) > case.layout(0).m          # the predicate splits regions


# ---------------------------------------------------------------- more than BS_BIG_MAX rows in one bucket
OVERSIZED_AGGS = [("SUM", "f64"), ("AVG", "f64"), ("MAX", "f64"), ("MIN", "f32"), ("SUM", "i64"), ("MIN", "i64"), ("COUNT", "i32"), ("AVG", "i32")]


@functools.lru_cache(maxsize=None)
def _oversized_case():
    from test_context_transitions import BS_BIG_MAX, _oversized

    a, b, _n = _oversized()
    table = tuple(x.astype(np.int64) for x in (b.chrom, b.start, b.end))
    assert int((table[1] < 4000).sum()) > BS_BIG_MAX
    case = Case("oversized", table, 1, 6100)
    small = Case("after-oversized", _table(np.random.default_rng(6101), 3_000, 450_000, 400), 1, 6102)
    return case, small, (a, b)


def _one_table_round(e, case, what):
    from giql_amd.engine import DeviceSide

    side = DeviceSide.from_numpy(case.chrom.astype(np.int32), case.start.astype(np.int32), case.end.astype(np.int32), device=DEV)
    cols = {k: (_t(v), _t(ok.astype(np.uint8))) for k, (v, ok) in case.cols.items()}
    stats = []
    for d in (0, DISTANCE):
        lay = case.layout(d)
        assert np.array_equal(e.cluster(side, 1, d).cpu().numpy(), lay.cluster_ids()), (what, "cluster", d)
        stats.append(e.stats())
        _rows_equal(e.merge(side, 1, d), lay, (what, "merge", d))
        stats.append(e.stats())
    out = e.merge_agg(side, 1, 0, [(f,) + cols[c] for f, c in OVERSIZED_AGGS])
    stats.append(e.stats())
    _rows_equal(out, case.layout(0), (what, "merge_agg"))
    for (func, col), got in zip(OVERSIZED_AGGS, out[4:]):
        _agg_equal(case, 0, func, col, got, (what, func, col))
    return stats, _bits(out)


def _oversized_round(e, expect_repeat):
    from test_context_transitions import _dev

    case, small, (a, b) = _oversized_case()
    stats, bits = _one_table_round(e, case, "the calls that meet the oversized bucket")
    assert all(st["sort_resorted"] == expect_repeat and not st["sort_local"] for st in stats), stats[0]
    stats, _b = _one_table_round(e, small, "the next one-table calls")
    assert all(st["sort_resorted"] == expect_repeat and not st["sort_local"] for st in stats), stats[0]
    ra, rb = e.inner_join(_dev(a), _dev(b), 1)
    assert np.array_equal(ora.sort_pairs(ra.cpu().numpy(), rb.cpu().numpy()), ora.sort_pairs(*ora.c_inner(a, b, "sweep")))
    st = e.stats()
    assert st["sort_resorted"] == expect_repeat and not st["sort_local"], st
    return bits


@functools.lru_cache(maxsize=None)
def _oversized_default_bits():
    e = _engine({})
    try:
        return _oversized_round(e, expect_repeat=False)
    finally:
        e.close()


@gpu
def test_oversized_bucket_on_a_fresh_default_context():
    """302,194 rows stay below the default context's 2^21-row floor: four passes, right rows, no repeat to report."""
    assert len(_oversized_default_bits()) == 2 * len(OVERSIZED_AGGS)


@gpu
@pytest.mark.parametrize("env", [LOCAL, {**LOCAL, "GIQL_HIP_LOCAL_BITS": "13"}], ids=["local", "local13"])
def test_oversized_bucket_repeats_the_call_with_four_passes(env):
    """A fresh context without the floor: the rows take the bucket stage, one bucket holds more than BS_BIG_MAX of them
    (GIQL_STATUS_RESORT at ``cluster_status``), the kernels behind the sort have run over unsorted rows by then, and
    ``with_order_fallback`` repeats the call with four passes -- for good on this context.  The repeat's aggregates
    are the default context's bit for bit."""
    e = _engine(env)
    try:
        bits = _oversized_round(e, expect_repeat=True)
    finally:
        e.close()
    _same_bits(bits, _oversized_default_bits(), "the default context's bits")
