"""Every operator at the top of the 32-bit axis and past it, against the C / Python oracle -- needs a GPU.

All chromosomes share one linear u32 axis (``k_chrom_offsets``, join_kernels.hip.h): key = base[c] + canonical
coordinate.  Spans summing to at most 2^32 - 1 run on one axis, the sentinel key of irregular rows one past the
last real key; past that a call returns GIQL_ERR_SPAN and the engine runs it chromosome group by group
(``HipEngine._wide`` over ``HipEngine._groups``; the groups' results are put together by ``giql_amd/wide.py``, whose
functions tests/test_wide_combine.py checks without a GPU).  Each axis class below is built from small seeded tables
whose COORDINATES sit at those edges, and every test first shows that its class was reached (the span a call reports,
or GIQL_ERR_SPAN from the C ABI), so a later change of layout cannot quietly turn it into a test of something easier.

Classes (canonical [lo, hi] per chromosome; span = hi - lo + 1):
  tight_top       [0, 2^31-1] + [1, 2^31-1]: exactly 2^32 - 1, real keys up to 0xFFFFFFFE next to the sentinel
  tight_over      [0, 2^31-1] twice: exactly 2^32, refused by the C ABI, answered by chromosome groups
  wide            five chromosomes of ~2^31 each (~1.07e10)
  one_chrom_max   [-2^31, 2^31-2]: one chromosome of span 2^32 - 1 with negative coordinates
  one_chrom_over  [-2^31, 2^31-1]: one chromosome of span 2^32, a clean error for every operator
  aligned_top     non-negative, exactly 255 blocks of 2^24 positions (the aligned axis at its limit)
  aligned_over    256 blocks: back on the tight axis
"""

import numpy as np
import pytest

from oracle import pyoracle as ora
from test_nearest_k import _triples

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOP = 2**32 - 1
B24 = 1 << 24

#: class -> canonical [lo, hi] per chromosome
LAYOUTS = {
    "tight_top": [(0, 2**31 - 1), (1, 2**31 - 1)],
    "tight_over": [(0, 2**31 - 1), (0, 2**31 - 1)],
    "wide": [(7 * c, 2**31 - 1 - 3 * c) for c in range(5)],
    "one_chrom_max": [(-2**31, 2**31 - 2)],
    "one_chrom_over": [(-2**31, 2**31 - 1)],
    "aligned_top": [(0, 127 * B24 + 5), (3, 99 * B24), (11, 26 * B24 + 77)],     # 128 + 100 + 27 = 255 blocks
    "aligned_over": [(0, 127 * B24 + 5), (3, 99 * B24), (11, 27 * B24 + 77)],    # 128 + 100 + 28 = 256 blocks
}
FITS = {"tight_top", "one_chrom_max", "aligned_top", "aligned_over"}   # one axis
GROUPED = {"tight_over", "wide"}                                          # one axis per chromosome group
ENCODINGS = [("0based", "half_open"), ("1based", "closed")]


def tight_span(name):
    return sum(hi - lo + 1 for lo, hi in LAYOUTS[name])


def aligned_blocks(name):
    return sum((hi >> 24) + 1 for _lo, hi in LAYOUTS[name])


def test_layouts_are_the_classes_they_name():
    assert tight_span("tight_top") == TOP and tight_span("tight_over") == 2**32
    assert tight_span("wide") > 1e10 and tight_span("one_chrom_max") == TOP and tight_span("one_chrom_over") == 2**32
    assert aligned_blocks("aligned_top") == 255 and aligned_blocks("aligned_over") == 256
    assert tight_span("aligned_over") < TOP


# ------------------------------------------------------------------ tables
def make_side(name, enc, n, seed, irregular=0, uniform=None, zero_length=True):
    """``n`` rows on the chromosomes of layout ``name`` in encoding ``enc``: a third in the lowest 65,536 positions
    of a chromosome, a third in its highest, a third anywhere; the first rows of each chromosome start at its ``lo``
    and end at its ``hi`` (so the span is exactly the layout's), some rows have length 0 (``zero_length``);
    ``irregular`` more rows with canonical end < start (sentinel key); ``uniform``: every regular row that long.
    Every RAW value lies in the chromosome's canonical range moved by the encoding's offsets, which keeps the span
    what the layout says."""
    so, eo = ora.ENCODING_OFFSETS[enc]
    r = np.random.default_rng(seed)
    ranges = LAYOUTS[name]
    nc = len(ranges)
    ch = r.integers(0, nc, n)
    ch[: 2 * nc] = np.repeat(np.arange(nc), 2)
    lo = np.array([ranges[c][0] for c in ch], np.int64)
    hi = np.array([ranges[c][1] for c in ch], np.int64)
    cs_max, ce_min = hi - eo + so, lo - so + eo          # raw start <= hi - eo, raw end >= lo - so
    where = r.integers(0, 3, n)
    cs = np.where(where == 0, lo + r.integers(0, 65536, n),
                  np.where(where == 1, hi - r.integers(0, 65536, n), lo + (r.random(n) * (hi - lo)).astype(np.int64)))
    ln = r.integers(1, 3000, n) if uniform is None else np.full(n, uniform)
    if uniform is None and zero_length:
        ln[r.random(n) < 0.05] = 0
    cs = np.clip(cs, np.maximum(lo, ce_min), cs_max - ln)
    ce = cs + ln
    lo_rows, hi_rows = np.arange(0, 2 * nc, 2), np.arange(1, 2 * nc, 2)
    fixed = 100 if uniform is None else uniform
    cs[lo_rows], ce[lo_rows] = lo[lo_rows], lo[lo_rows] + fixed     # starts at lo
    cs[hi_rows], ce[hi_rows] = hi[hi_rows] - fixed, hi[hi_rows]     # ends at hi
    if irregular:
        ic = r.integers(0, nc, irregular)
        ilo = np.array([ranges[c][0] for c in ic], np.int64) - so + eo
        ihi = np.array([ranges[c][1] for c in ic], np.int64) - eo + so
        ics = np.where(r.random(irregular) < 0.5, ihi - r.integers(0, 65536, irregular),
                       ilo + (r.random(irregular) * (ihi - ilo)).astype(np.int64))
        ics = np.clip(ics, ilo + 2000, ihi)
        ch = np.concatenate([ch, ic])
        cs = np.concatenate([cs, ics])
        ce = np.concatenate([ce, ics - r.integers(1, 1000, irregular)])
    raw_s, raw_e = cs - so, ce - eo
    assert raw_s.min() >= -2**31 and raw_e.max() < 2**31
    return ora.Side(ch.astype(np.int32), raw_s.astype(np.int32), raw_e.astype(np.int32), so, eo)


def dev(side: ora.Side):
    from giql_amd.engine import DeviceSide

    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.int32)).to("cuda:0")
    return DeviceSide(t(side.chrom), t(side.start), t(side.end), side.start_off, side.end_off)


# ----------------------------------------------------------------- contexts
CONTEXTS = {"default": {}, "local": {"GIQL_HIP_LOCAL_MIN_ROWS": "1"},
            "narrow": {"GIQL_HIP_LOCAL_MIN_ROWS": "1", "GIQL_HIP_LOCAL_BITS": "13"}}


@pytest.fixture(scope="module", params=list(CONTEXTS))
def eng(request):
    """A default context, one that sorts in three stages (tests/test_sort_stages.py's ``eng_local``) and one with
    13-bit buckets (tests/test_bucket_width.py's ``eng_narrow``): the top bucket is another key range in each."""
    from giql_amd.engine import HipEngine

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    with pytest.MonkeyPatch.context() as mp:
        for k, v in CONTEXTS[request.param].items():
            mp.setenv(k, v)
        e = HipEngine(0)
    e.kind = request.param
    yield e
    e.close()


def assert_span_error(fn):
    from giql_amd import _lib

    with pytest.raises(_lib.GiqlHipError) as ei:
        fn()
    assert ei.value.code == _lib.GIQL_ERR_SPAN


def reach(eng, name, a, b):
    """Show the class was reached: a fitting layout reports its span, a wider one is refused by the C ABI."""
    da, db = dev(a), dev(b)
    n = len(LAYOUTS[name])
    if name in FITS:
        eng._count_once(da, db, n)
        assert eng.stats()["span"] == tight_span(name), (name, eng.stats()["span"])
    else:
        assert_span_error(lambda: eng._count_once(da, db, n))
        assert_span_error(lambda: eng.inner_plan(da, db, n))
        if name in GROUPED:
            assert sum(eng.chrom_spans(da, db, n)) == tight_span(name)
    return da, db, n


def host(t):
    return t.cpu().numpy()


JOIN_CLASSES = [c for c in LAYOUTS if c != "one_chrom_over"]


# ---------------------------------------------------------------- the joins
@pytest.mark.parametrize("enc", ENCODINGS, ids=lambda e: e[0])
@pytest.mark.parametrize("name", JOIN_CLASSES)
def test_inner_semi_anti_count(eng, name, enc):
    a = make_side(name, enc, 2500, 1, irregular=150)
    b = make_side(name, enc, 4000, 2, irregular=150)
    da, db, n = reach(eng, name, a, b)
    if name == "tight_top":   # real keys in the top 65,536, next to the sentinel; rows ending at key 0xFFFFFFFE
        base1 = 2**31 - 1
        top = (b.chrom == 1) & (b.ce + base1 >= TOP - 65536) & (b.ce >= b.cs)
        assert top.sum() > 500 and (b.ce[b.chrom == 1] + base1 == TOP - 1).any() and ((b.ce == b.cs) & top).any()
    for x, y, dx, dy in ((a, b, da, db), (b, a, db, da)):     # the larger side as B, then as A
        ra, rb = eng.inner_join(dx, dy, n)
        st = eng.stats()
        assert st["sort_local"] == (eng.kind != "default") and (eng.kind != "narrow" or st["bucket_bits"] == 13), st
        got = ora.sort_pairs(host(ra), host(rb))
        want_a, want_b = ora.c_inner(x, y)
        assert got.shape[0] > 1000 and np.array_equal(got, ora.sort_pairs(want_a, want_b))
        assert eng.pairs_checksum(ra, rb) == ora.c_pairs_checksum(want_a, want_b)
    assert np.array_equal(host(eng.semi_join(da, db, n)), ora.c_semi_anti(a, b, False))
    assert np.array_equal(host(eng.anti_join(da, db, n)), ora.c_semi_anti(a, b, True))
    assert np.array_equal(host(eng.count_overlaps(da, db, n)), ora.c_count(a, b))


@pytest.mark.parametrize("enc", ENCODINGS, ids=lambda e: e[0])
@pytest.mark.parametrize("name", JOIN_CLASSES)
def test_inner_uniform_form(eng, name, enc):
    a = make_side(name, enc, 3000, 3)
    b = make_side(name, enc, 2000, 4, uniform=700)
    da, db, n = reach(eng, name, a, b)
    ra, rb = eng.inner_join(da, db, n)
    if name in FITS:
        assert eng.stats()["join_form"] in ("uniform_a", "uniform_b")
    want = ora.sort_pairs(*ora.c_inner(a, b))
    assert want.shape[0] > 500 and np.array_equal(ora.sort_pairs(host(ra), host(rb)), want)


# ------------------------------------------------------------ LEFT OUTER
@pytest.mark.parametrize("enc", ENCODINGS, ids=lambda e: e[0])
@pytest.mark.parametrize("name", sorted(GROUPED))
def test_left_join_by_chromosome_groups(eng, name, enc):
    """The groups' pairs come back in tensors of exactly their length: ``left_join`` pads a copy with room."""
    import _left_ref as R

    a = make_side(name, enc, 2500, 23, irregular=150)
    b = make_side(name, enc, 4000, 24, irregular=150)
    da, db, n = reach(eng, name, a, b)
    ra, rb = eng.left_join(da, db, n)
    want = R.left_rows(a, b)
    assert (want[:, 1] >= 0).sum() > 1000 and (want[:, 1] < 0).sum() > 100
    assert ra.dtype == rb.dtype == torch.int32 and np.array_equal(R.sort_rows(host(ra), host(rb)), want)


# -------------------------------------------------------------- NEAREST
def _same_targets(b, idx, oi):
    m = oi >= 0
    return (np.array_equal(idx >= 0, m) and np.array_equal(b.start[idx[m]], b.start[oi[m]])
            and np.array_equal(b.end[idx[m]], b.end[oi[m]]))


@pytest.mark.parametrize("enc", ENCODINGS, ids=lambda e: e[0])
@pytest.mark.parametrize("name", JOIN_CLASSES)
def test_nearest(eng, name, enc):
    from giql_amd import _lib

    a = make_side(name, enc, 2500, 5)
    b = make_side(name, enc, 3000, 6)
    da, db, n = reach(eng, name, a, b)
    for signed, md in ((False, None), (True, None), (False, 5000), (True, 2**31)):
        idx, dist = eng.nearest(da, db, n, signed=signed, max_distance=md)
        oi, od = ora.c_nearest_k1(a, b, signed=signed, max_distance=md)
        assert np.array_equal(host(dist), od) and _same_targets(b, host(idx), oi), (signed, md)
        if name in GROUPED:   # nearest32's contract: a genome wider than 32 bits belongs to nearest()
            assert_span_error(lambda: eng.nearest32(da, db, n, signed=signed, max_distance=md))
            continue
        if np.abs(od).max() < 2**31:
            rec = host(eng.nearest32(da, db, n, signed=signed, max_distance=md))
            assert np.array_equal(rec[:, 1].astype(np.int64), od) and _same_targets(b, rec[:, 0], oi)
        else:
            with pytest.raises(_lib.GiqlHipError):
                eng.nearest32(da, db, n, signed=signed, max_distance=md)


@pytest.mark.parametrize("k", [2, 17])
@pytest.mark.parametrize("enc", ENCODINGS, ids=lambda e: e[0])
@pytest.mark.parametrize("name", JOIN_CLASSES)
def test_nearest_k(eng, name, enc, k):
    a = make_side(name, enc, 1500, 7)
    b = make_side(name, enc, 2000, 8)
    da, db, n = reach(eng, name, a, b)
    if name in GROUPED:
        assert_span_error(lambda: eng._nearest_k_once(da, db, n, k))
    for signed, md in ((False, None), (True, 20_000)):
        idx, dist = eng.nearest_k(da, db, n, k, signed=signed, max_distance=md)
        if name in FITS:
            assert eng.stats()["span"] == tight_span(name)
        oi, od = ora.c_nearest_k(a, b, k, signed=signed, max_distance=md)
        idx, dist = host(idx), host(dist)
        assert np.array_equal(idx >= 0, oi >= 0) and np.array_equal(dist, od)
        assert _triples(idx, dist, b) == _triples(oi, od, b)


# ------------------------------------------------------- CLUSTER / MERGE
# raw coordinates (offsets 0): the 0-based half-open tables, where raw = canonical and the class is exact
RAW_ENC = ("0based", "half_open")


def _reach_raw(eng, name, s):
    d = dev(s)
    n = len(LAYOUTS[name])
    if name in FITS:
        eng._cluster_once(d, n, 0)
        assert eng.stats()["span"] == tight_span(name)
    else:
        assert_span_error(lambda: eng._cluster_once(d, n, 0))
    return d, n


@pytest.mark.parametrize("distance", [0, 2**31])
@pytest.mark.parametrize("name", JOIN_CLASSES)
def test_cluster_merge(eng, name, distance):
    s = make_side(name, RAW_ENC, 5000, 9)
    d, n = _reach_raw(eng, name, s)
    ids = host(eng.cluster(d, n, distance))
    assert np.array_equal(ids, ora.c_cluster(s, distance))
    # every partition opens with cluster 1, however far the distance reaches across the axis
    for c in range(n):
        first = np.lexsort((np.arange(s.n), s.start, s.chrom != c))[0]
        assert s.chrom[first] == c and ids[first] == 1
    got = list(zip(*(host(t) for t in eng.merge(d, n, distance))))
    assert got == list(zip(*ora.c_merge(s, distance)))


def _payload(seed, m):
    r = np.random.default_rng(seed)
    col = np.repeat(r.integers(0, 3, m // 40 + 1), 40)[:m].astype(np.int32)[r.permutation(m)]
    col[r.random(m) < 0.1] = 0
    valid = (r.random(m) > 0.05).astype(np.uint8)
    return col, valid


@pytest.mark.parametrize("distance", [0, 2**31])
@pytest.mark.parametrize("name", JOIN_CLASSES)
def test_cluster_merge_predicate(eng, name, distance):
    s = make_side(name, RAW_ENC, 6000, 10)
    # neighbours in start order: one run of rows per chromosome where the predicate decides
    d, n = _reach_raw(eng, name, s)
    col, valid = _payload(11, s.n)
    tc, tv = torch.from_numpy(col).cuda(), torch.from_numpy(valid).cuda()
    preds = [(("a", tc, tv), "=", ("b", tc, tv))]
    if name in GROUPED:
        assert_span_error(lambda: eng._cluster_pred_once(d, n, distance, preds))
        assert_span_error(lambda: eng._merge_once(d, n, distance, preds))
    holds = lambda i, j: bool(valid[i]) and bool(valid[j]) and col[i] == col[j]
    want = ora.py_cluster_predicate(s.chrom.tolist(), s.start.tolist(), s.end.tolist(), distance, holds)
    assert np.array_equal(host(eng.cluster(d, n, distance, preds=preds)), want)
    assert len(set(zip(s.chrom.tolist(), want.tolist()))) > 100
    regions = {}
    for c, cid, st, en in zip(s.chrom.tolist(), want.tolist(), s.start.tolist(), s.end.tolist()):
        g = regions.setdefault((c, cid), [st, en, 0])
        g[0], g[1], g[2] = min(g[0], st), max(g[1], en), g[2] + 1
    want_m = sorted((c, g[0], g[1], g[2]) for (c, _), g in regions.items())
    got = [tuple(int(x) for x in r) for r in zip(*(host(t) for t in eng.merge(d, n, distance, preds=preds)))]
    assert sorted(got) == want_m
    assert [(r[0], r[1]) for r in got] == sorted((r[0], r[1]) for r in got)   # ordered by (chrom, start)


# ------------------------------------------------------------- GROUP BY
@pytest.mark.parametrize("enc", ENCODINGS, ids=lambda e: e[0])
@pytest.mark.parametrize("name", JOIN_CLASSES)
def test_group_rows_segment_sum(eng, name, enc):
    s0 = make_side(name, enc, 4000, 12, irregular=100)
    r = np.random.default_rng(13)
    pick = np.concatenate([np.arange(s0.n), r.integers(0, s0.n, 5000)])   # every row, and duplicate keys
    s = ora.Side(s0.chrom[pick], s0.start[pick], s0.end[pick], s0.start_off, s0.end_off)
    d = dev(s)
    n = len(LAYOUTS[name])
    # the kernel groups RAW coordinates, whose span may differ from the canonical one by the offsets
    raw = np.concatenate([s.start, s.end]).astype(np.int64)
    ch = np.concatenate([s.chrom, s.chrom])
    raw_span = sum(int(raw[ch == c].max() - raw[ch == c].min() + 1) for c in range(n))
    if enc == RAW_ENC:
        assert raw_span == tight_span(name)
    if raw_span > TOP:
        assert_span_error(lambda: eng._group_rows_once(d, n))
    gid, rep = eng.group_rows(d, n)
    gid, rep = host(gid), host(rep)
    keys = np.stack([s.chrom, s.start, s.end], 1).astype(np.int64)
    uniq, inv = np.unique(keys, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    assert np.array_equal(gid, inv)
    assert np.array_equal(keys[rep], uniq)
    vals = r.integers(-2**40, 2**40, s.n).astype(np.int64)
    sums = host(eng.segment_sum(torch.from_numpy(vals).cuda(), torch.from_numpy(gid).cuda(), rep.size))
    want = np.zeros(uniq.shape[0], np.int64)
    np.add.at(want, inv, vals)
    assert np.array_equal(sums, want)


# -------------------------------------------------------------- DISJOIN
def _disjoin_want(t, r=None):
    """``brute_force_arrays`` (anchored row by row in tests/test_disjoin.py) on the canonical columns, the pieces
    back in the target's encoding."""
    from _disjoin_ref import brute_force_arrays

    cols = [t.chrom.astype(np.int64), t.cs.astype(np.int64), t.ce.astype(np.int64)]
    if r is not None:
        cols += [r.chrom.astype(np.int64), r.cs.astype(np.int64), r.ce.astype(np.int64)]
    want = brute_force_arrays(*cols)
    want[:, 1] -= t.start_off
    want[:, 2] -= t.end_off
    return want


@pytest.mark.parametrize("mode", ["self", "reference"])
@pytest.mark.parametrize("enc", ENCODINGS, ids=lambda e: e[0])
@pytest.mark.parametrize("name", JOIN_CLASSES)
def test_disjoin(eng, name, enc, mode):
    """``k_dj_events`` writes real keys with no sentinel: up to 0xFFFFFFFE at span 2^32 - 1, in the top bucket of
    every sort form."""
    t = make_side(name, enc, 2500, 18, zero_length=True)
    r = make_side(name, enc, 4000, 19, zero_length=True) if mode == "reference" else None
    dt, dr = dev(t), None if r is None else dev(r)
    n = len(LAYOUTS[name])
    want = _disjoin_want(t, r)
    assert want.shape[0] > 2000
    if name == "tight_top":      # events in the top 65,536 keys, one of them 0xFFFFFFFE
        ref = r if r is not None else t
        key = ref.ce[ref.chrom == 1].astype(np.int64) + 2**31 - 1
        assert key.max() == TOP - 1 and (key >= TOP - 65536).sum() > 300
    if name in FITS:
        got = eng._disjoin_once(dt, dr, n)
        st = eng.stats()
        assert st["span"] == tight_span(name), (name, st["span"])
        assert st["sort_local"] == (eng.kind != "default") and (eng.kind != "narrow" or st["bucket_bits"] == 13), st
    else:
        assert_span_error(lambda: eng._disjoin_once(dt, dr, n))
        got = eng.disjoin(dt, dr, n)
    got = np.stack([host(x) for x in got], 1).astype(np.int64)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert not eng.stats()["sort_resorted"]


# -------------------------------------------------------------- CONTAINS / WITHIN
CONTAIN_LAYOUTS = ["tight_top", "one_chrom_max", "tight_over", "wide"]   # (tests/test_contain_gpu.py: the general form there)
CONTAIN_L = 60


def contain_sides(name, form):
    """Outer rows with irregular ones among them; the inner side irregular rows too (general form) or every row
    CONTAIN_L long.  ``make_side`` ends one row of each side exactly at the top of every chromosome: the inner one
    ([hi - 100, hi), or [hi - CONTAIN_L, hi)) lies inside the outer one ([hi - 100, hi)) with equal ends."""
    enc = ("1based", "closed")
    a = make_side(name, enc, 1500, 21, irregular=60)
    b = make_side(name, enc, 2500, 22, irregular=60) if form == "general" else make_side(name, enc, 2500, 22, uniform=CONTAIN_L)
    return a, b


@pytest.mark.parametrize("form", ["general", "uniform_b"])
@pytest.mark.parametrize("name", CONTAIN_LAYOUTS)
def test_contain(eng, name, form):
    """Both forms of the containment join with keys up to 0xFFFFFFFE on every sort form: the general form's
    ``inner end <= outer end`` and the uniform form's shifted upper key at the largest regular key."""
    import _contain_ref as C

    a, b = contain_sides(name, form)
    da, db, n = dev(a), dev(b), len(LAYOUTS[name])
    want = C.contain_pairs(a.chrom, a.cs, a.ce, b.chrom, b.cs, b.ce)
    hi = LAYOUTS[name][n - 1][1]
    top_o = np.nonzero((a.chrom == n - 1) & (a.ce == hi) & (a.cs < a.ce))[0]
    top_i = np.nonzero((b.chrom == n - 1) & (b.ce == hi) & (b.cs < b.ce))[0]
    assert want.shape[0] > 50 and (np.isin(want[:, 0], top_o) & np.isin(want[:, 1], top_i)).any()
    if name in ("tight_top", "one_chrom_max"):      # both rows end at key 0xFFFFFFFE
        base = sum(h - l + 1 for l, h in LAYOUTS[name][: n - 1]) - LAYOUTS[name][n - 1][0]
        assert hi + base == TOP - 1
    if name in FITS:
        ro, ri = eng._contain_once(da, db, n)
        st = eng.stats()
        assert st["span"] == tight_span(name) and st["join_form"] == form, (name, st["span"], st["join_form"])
        assert st["sort_local"] == (eng.kind != "default") and (eng.kind != "narrow" or st["bucket_bits"] == 13), st
    else:
        assert_span_error(lambda: eng.contain_plan(da, db, n))
        ro, ri = eng.contain_join(da, db, n)
    got = C.sort_pairs(np.stack([host(ro), host(ri)], 1))
    assert eng.stats()["n_out"] > 0 and np.array_equal(got, want)
    assert not eng.stats()["sort_resorted"]


@pytest.mark.parametrize("enc", ENCODINGS, ids=lambda e: e[0])
def test_disjoin_one_chromosome_past_32_bits_is_a_clean_error(eng, enc):
    from giql_amd import _lib

    t = make_side("one_chrom_over", enc, 2000, 20)
    r = make_side("one_chrom_over", enc, 2000, 21)
    for dr in (None, dev(r)):
        assert_span_error(lambda: eng._disjoin_once(dev(t), dr, 1))
        with pytest.raises((ValueError, _lib.GiqlHipError)):
            eng.disjoin(dev(t), dr, 1)
    small = make_side("aligned_top", enc, 600, 22)      # the context answers afterwards
    got = np.stack([host(x) for x in eng.disjoin(dev(small), None, 3)], 1).astype(np.int64)
    assert np.array_equal(got, _disjoin_want(small))


# ---------------------------------------------------------------- index
@pytest.mark.parametrize("enc", ENCODINGS, ids=lambda e: e[0])
@pytest.mark.parametrize("name", JOIN_CLASSES)
def test_index(eng, name, enc):
    from giql_amd import _lib

    a = make_side(name, enc, 2500, 14, zero_length=False)   # (an indexed join takes no irregular row)
    b = make_side(name, enc, 4000, 15, zero_length=False)
    da, db = dev(a), dev(b)
    n = len(LAYOUTS[name])
    if name != "aligned_top":
        with pytest.raises(_lib.GiqlHipError) as ei:
            eng.index_create(db, n)
        allowed = (_lib.GIQL_ERR_STATE, _lib.GIQL_ERR_SPAN) if name in GROUPED else (_lib.GIQL_ERR_STATE,)
        assert ei.value.code in allowed
        if name == "aligned_over":   # the tight axis instead: the span the join reports
            eng.inner_join(da, db, n)
            assert eng.stats()["span"] == tight_span(name)
        return
    idx = eng.index_create(db, n)
    try:
        assert idx.span == 255 << 24 and eng.stats()["span"] == 255 << 24
        ra, rb = eng.inner_join_indexed(da, idx)
        want = ora.sort_pairs(*ora.c_inner(a, b))
        assert want.shape[0] > 1000 and np.array_equal(ora.sort_pairs(host(ra), host(rb)), want)
    finally:
        idx.close()


# ------------------------------------------------- one chromosome of 2^32
@pytest.mark.parametrize("enc", ENCODINGS, ids=lambda e: e[0])
def test_one_chromosome_past_32_bits_is_a_clean_error(eng, enc):
    from giql_amd import _lib

    a = make_side("one_chrom_over", enc, 2000, 16)
    b = make_side("one_chrom_over", enc, 2000, 17)
    da, db, n = reach(eng, "one_chrom_over", a, b)
    bad = (ValueError, _lib.GiqlHipError)
    calls = [lambda: eng.inner_join(da, db, n), lambda: eng.semi_join(da, db, n), lambda: eng.anti_join(da, db, n),
             lambda: eng.count_overlaps(da, db, n), lambda: eng.nearest(da, db, n), lambda: eng.nearest32(da, db, n),
             lambda: eng.nearest_k(da, db, n, 3), lambda: eng.index_create(db, n)]
    if enc == RAW_ENC:   # raw coordinates span 2^32 as well
        tc = torch.zeros(a.n, dtype=torch.int32, device="cuda:0")
        preds = [(("a", tc), "=", ("b", tc))]
        calls += [lambda: eng.cluster(da, n), lambda: eng.merge(da, n), lambda: eng.group_rows(da, n),
                  lambda: eng.cluster(da, n, preds=preds), lambda: eng.merge(da, n, preds=preds)]
    for call in calls:
        with pytest.raises(bad):
            call()


# ------------------------------------------------------------- execute()
HG38 = [248_956_422, 242_193_529, 198_295_559, 190_214_555, 181_538_259, 170_805_979, 159_345_973, 145_138_636,
        138_394_717, 133_797_422, 135_086_622, 133_275_309, 114_364_328, 107_043_718, 101_991_189, 90_338_345,
        83_257_441, 80_373_285, 58_617_616, 64_444_167, 46_709_983, 50_818_468, 156_040_895, 57_227_415]


def genome_table(r, lens, n, tag, strands="+-"):
    """Rows on chromosomes ``chr1..`` of the given lengths, every chromosome reaching its end; a dense corner at
    the start of each so that rows meet."""
    nc = len(lens)
    ch = r.integers(0, nc, n)
    ch[:nc] = np.arange(nc)
    st = np.array([int(r.integers(0, lens[c] - 5000)) for c in ch], np.int64)
    dense = r.random(n) < 0.5
    st[dense] = r.integers(0, 200_000, int(dense.sum()))
    st[:nc] = [lens[c] - 5000 for c in range(nc)]
    en = st + r.integers(1, 4000, n)
    pa = pytest.importorskip("pyarrow")
    return pa.table({"chrom": pa.array([f"chr{int(c) + 1}" for c in ch]), "start": pa.array(st, pa.int32()),
                     "end": pa.array(en, pa.int32()), "name": pa.array([f"{tag}{i}" for i in range(n)]),
                     "strand": pa.array([strands[int(k)] for k in r.integers(0, len(strands), n)])}), ch


def _side_of(tbl, codes):
    return ora.Side(codes.astype(np.int32), tbl.column("start").to_numpy(), tbl.column("end").to_numpy())


def test_execute_nearest_k3_on_a_genome_wider_than_32_bits():
    from giql_amd.execute import execute

    r = np.random.default_rng(21)
    lens = [600_000_000 + 1000 * c for c in range(8)]
    assert sum(lens) > 2**32
    (peaks, ca), (genes, cb) = genome_table(r, lens, 3000, "p"), genome_table(r, lens, 4000, "g")
    q = ('SELECT a.name, b.start AS bs, b."end" AS be, b.distance AS d FROM peaks a CROSS JOIN LATERAL '
         "NEAREST(genes, reference := a.interval, k := 3) b")
    out = execute(q, {"peaks": peaks, "genes": genes}, giql_tables=["peaks", "genes"])
    a, b = _side_of(peaks, ca), _side_of(genes, cb)
    oi, od = ora.c_nearest_k(a, b, 3)
    want = {f"p{i}": t for i, t in enumerate(_triples(oi, od, b))}
    got = {}
    for row in out.to_pylist():
        got.setdefault(row["name"], []).append((row["d"], row["bs"], row["be"]))
    assert out.num_rows == 3 * 3000 and got == want


def test_execute_stranded_nearest_k2_on_hg38():
    from giql_amd.execute import execute

    r = np.random.default_rng(22)
    (peaks, _), (genes, _) = genome_table(r, HG38, 3000, "p", "+-+-."), genome_table(r, HG38, 4000, "g", "+-+-.")
    q = ('SELECT a.name, b.name AS g, b.distance AS d FROM peaks a CROSS JOIN LATERAL '
         "NEAREST(genes, reference := a.interval, k := 2, stranded := true, signed := true) b")
    out = execute(q, {"peaks": peaks, "genes": genes}, giql_tables=["peaks", "genes"])
    got = {}
    for row in out.to_pylist():
        got.setdefault(row["name"], []).append((row["g"], row["d"]))
    P, G = peaks.to_pylist(), genes.to_pylist()
    gi = {g["name"]: g for g in G}
    assert sum(p["strand"] == "." for p in P[:300]) > 20
    for p in P[:300]:   # brute force on a sample
        cand = []
        for g in G:
            if g["chrom"] != p["chrom"] or g["strand"] != p["strand"]:
                continue
            if p["strand"] == ".":   # the distance CASE is NULL: ORDER BY falls through to (start, end)
                cand.append(((0, g["start"], g["end"]), None))
                continue
            if g["start"] < p["end"] and g["end"] > p["start"]:
                d = 0
            elif g["end"] <= p["start"]:
                d = -(p["start"] - g["end"] + 1)
            else:
                d = g["start"] - p["end"] + 1
            cand.append(((abs(d), g["start"], g["end"]), d * (-1 if p["strand"] == "-" else 1)))
        cand.sort(key=lambda c: c[0])
        have = got.get(p["name"], [])
        assert [d for _g, d in have] == [d for _k, d in cand[:2]], p
        assert [(gi[g]["start"], gi[g]["end"]) for g, _d in have] == [k[1:] for k, _d in cand[:2]], p


def _features(r, n):
    pa = pytest.importorskip("pyarrow")
    tbl, ch = genome_table(r, HG38, n, "f")
    depth = r.integers(0, 3, n)
    valid = r.random(n) > 0.05
    return tbl.append_column("depth", pa.array(depth, pa.int64(), mask=~valid)), ch, depth, valid


def _predicate_ids(tbl, ch, depth, valid, distance):
    strand = tbl.column("strand").to_pylist()
    part = list(zip(ch.tolist(), strand))
    holds = lambda i, j: bool(valid[i]) and bool(valid[j]) and depth[i] == depth[j]
    ids = ora.py_cluster_predicate(part, tbl.column("start").to_pylist(), tbl.column("end").to_pylist(), distance,
                                   holds)
    return part, ids


def test_execute_stranded_cluster_and_merge_with_a_predicate_on_hg38(monkeypatch):
    """(chrom, strand) partitions on hg38 make an axis of ~6.2e9: the engine runs the predicate CLUSTER / MERGE
    one chromosome group at a time."""
    from giql_amd.engine import HipEngine
    from giql_amd.execute import execute

    r = np.random.default_rng(23)
    tbl, ch, depth, valid = _features(r, 12_000)
    grouped = []
    groups = HipEngine._groups

    def spy(self, *args):
        for g in groups(self, *args):
            grouped.append(int(g[0].n))
            yield g

    monkeypatch.setattr(HipEngine, "_groups", spy)
    q = "SELECT *, CLUSTER(interval, 100, stranded := true, predicate := depth = PREV(depth)) AS cid FROM t"
    out = execute(q, {"t": tbl}, giql_tables=["t"])
    assert len(grouped) > 1 and sum(grouped) == tbl.num_rows   # the whole table did not fit one axis
    part, ids = _predicate_ids(tbl, ch, depth, valid, 100)
    assert out.column("cid").to_pylist() == ids.tolist()
    assert out.column("name").to_pylist() == tbl.column("name").to_pylist()

    out = execute("SELECT MERGE(interval, 100, stranded := true, predicate := depth = PREV(depth)), COUNT(*) AS n "
                  "FROM t", {"t": tbl}, giql_tables=["t"])
    regions = {}
    for (c, s), cid, st, en in zip(part, ids.tolist(), tbl.column("start").to_pylist(), tbl.column("end").to_pylist()):
        g = regions.setdefault((c, s, cid), [st, en, 0])
        g[0], g[1], g[2] = min(g[0], st), max(g[1], en), g[2] + 1
    want = sorted((f"chr{c + 1}", s, g[0], g[1], g[2]) for (c, s, _), g in regions.items())
    got = list(zip(*(out.column(k).to_pylist() for k in ("chrom", "strand", "start", "end", "n"))))
    assert sorted(got) == want and len(want) > 1000 and sum(grouped) == 2 * tbl.num_rows


def test_execute_count_overlaps_grouped_on_a_genome_wider_than_32_bits(monkeypatch):
    pa = pytest.importorskip("pyarrow")
    from giql_amd.engine import HipEngine
    from giql_amd.execute import execute

    r = np.random.default_rng(24)
    lens = [2**31 - 1000 * (c + 1) for c in range(3)]
    (peaks, ca), (genes, cb) = genome_table(r, lens, 3000, "p"), genome_table(r, lens, 5000, "g")
    peaks = pa.concat_tables([peaks, peaks.slice(0, 500)])   # duplicate keys
    ca = np.concatenate([ca, ca[:500]])
    grouped = []
    group_rows = HipEngine.group_rows

    def spy(self, s, n_chrom):
        out = group_rows(self, s, n_chrom)
        grouped.append(int(out[1].shape[0]))
        return out

    monkeypatch.setattr(HipEngine, "group_rows", spy)
    q = ('SELECT a.chrom, a.start, a."end", COUNT(b.chrom) AS n FROM peaks a '
         'LEFT JOIN genes b ON a.interval INTERSECTS b.interval GROUP BY a.chrom, a.start, a."end"')
    out = execute(q, {"peaks": peaks, "genes": genes}, giql_tables=["peaks", "genes"])
    assert len(grouped) == 1   # the GPU GROUP BY answered; the host one is only a safety net
    counts = ora.c_count(_side_of(peaks, ca), _side_of(genes, cb))
    ungrouped = pa.table({"chrom": peaks.column("chrom"), "start": peaks.column("start"),
                          "end": peaks.column("end"), "n": pa.array(counts, pa.int64())})
    want = ungrouped.group_by(["chrom", "start", "end"], use_threads=False).aggregate([("n", "sum")])
    want = sorted(zip(*(want.column(k).to_pylist() for k in ("chrom", "start", "end", "n_sum"))))
    got = sorted(zip(*(out.column(k).to_pylist() for k in ("chrom", "start", "end", "n"))))
    assert got == want and grouped[0] == len(want) and sum(w[3] for w in want) > 1000
