"""DISJOIN's kernels path by path, and its event sort under every sort form -- needs a GPU.

``tests/_disjoin_ref.py`` builds one table pair per path of ``k_dj_fill`` / ``k_dj_count``
(``giql_amd/csrc/disjoin_kernels.hip.h``); ``tests/test_disjoin.py`` shows without a GPU that each reaches the path
it names (a numpy mirror of the fill's tiles) and that the vectorised brute force used here equals the row-by-row
one on all of them.  Integers throughout: every comparison is exact.

The sort forms.  DISJOIN sorts its 2n (key, id) events with ``run_sort_onesweep``.  Of the switches of DESIGN.md
section 6b that sort honours for a (key, id) sort: GIQL_HIP_LOCAL_MIN_ROWS, GIQL_HIP_LOCAL_BITS,
GIQL_HIP_NO_LOCAL_SORT, GIQL_HIP_OS_ORDER, GIQL_HIP_OS_VARIANT (which also turns the three-stage form off),
GIQL_HIP_OS_HELP_AFTER and, at the call's read-back, GIQL_HIP_INJECT_TIMEOUT -- each has a context in ``FORMS``.
GIQL_HIP_LOCAL_MIN / MAX_BUCKET_ROWS and GIQL_HIP_NO_NARROW_BUCKETS act through the density of the context's
previous call (``guess.last_span``), which DISJOIN reads and never sets: the walks of
``tests/test_context_transitions.py`` run DISJOIN on such a context.  GIQL_HIP_SORT=classic, NO_UNIFORM,
NO_SPAN_HIST, NO_COARSE_B and NO_FUSE_COUNT are not read on this path.
"""

import functools

import numpy as np
import pytest

import _disjoin_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
SENTINEL = -77


def _engine(env):
    from giql_amd.engine import HipEngine

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    with pytest.MonkeyPatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        return HipEngine(0)


@pytest.fixture(scope="module")
def eng():
    e = _engine({})
    yield e
    e.close()


def _side(cols, enc=R.HALF_OPEN):
    from giql_amd.engine import DeviceSide

    return DeviceSide.from_numpy(*(np.asarray(x, np.int32) for x in cols), enc, device=DEV)


def _sides(case):
    return _side(case.t, case.t_enc), None if case.r is None else _side(case.r, case.r_enc)


def _rows(parent, ds, de):
    return np.stack([parent.cpu().numpy(), ds.cpu().numpy(), de.cpu().numpy()], 1).astype(np.int64)


def _same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), what


# ---- the raw ABI: plan and fill as two calls, the fill into buffers of the test's own making
_plan, _fill = R.plan_raw, R.fill_raw


def _buffers(total, shifts, pad=64):
    """Three views of ``total`` int32 slots inside larger sentinel-filled allocations, ``shifts[i]`` slots in: 4 keeps
    the view 16-byte aligned, 1 (a ``[1:]`` view) does not."""
    bigs = [torch.full((total + pad + s,), SENTINEL, dtype=torch.int32, device=DEV) for s in shifts]
    views = [b[s:s + total] for b, s in zip(bigs, shifts)]
    for v, s in zip(views, shifts):
        assert (v.data_ptr() % 16 == 0) == (s % 4 == 0)
    return bigs, views


def _sentinels_untouched(bigs, shifts, total):
    return all(bool((b[:s] == SENTINEL).all()) and bool((b[s + total:] == SENTINEL).all()) for b, s in zip(bigs, shifts))


PATHS = R.path_cases()
COVERAGE = R.coverage_cases()


@functools.lru_cache(maxsize=None)
def _expected(cid):
    return PATHS[cid][0].expected()


# ---------------------------------------------------------------- k_dj_fill / k_dj_count, path by path
@pytest.mark.parametrize("cid", list(PATHS))
def test_fill_path(eng, cid):
    case = PATHS[cid][0]
    target, reference = _sides(case)
    _same(_rows(*eng.disjoin(target, reference, case.n_chrom)), _expected(cid), cid)
    assert eng.stats()["n_out"] == len(_expected(cid))


@pytest.mark.parametrize("cid", ["unstaged-5000", "cap-plus-one"])
def test_unstaged_tile_in_self_mode(eng, cid):
    """Self mode leaves a piece for every live row: only zero-length targets make a tile span more than DJ_OFF_CAP
    rows there.  The path cases' targets alone, their zero-piece rows as points."""
    cnt = PATHS[cid][1]
    base = R.case_from_counts(cid, cnt, seed=3, zero="point")
    case = R.Case(cid + "-self", base.t)
    assert not any(t["staged"] for t in R.fill_mirror(case.counts())) and int((case.counts() == 0).sum()) >= 4095
    _same(_rows(*eng.disjoin(_side(case.t), None, 1)), case.expected(), case.id)


SHIFTS = {"aligned": (4, 4, 4), "parent": (1, 4, 4), "start": (4, 1, 4), "end": (4, 4, 1), "all": (1, 1, 1)}


@pytest.mark.parametrize("cid", ["total-4097", "total-5", "total-mod-4-is-3", "parent-straddles-five-tiles",
                                 "unstaged-5000", "unstaged-second-tile"])
def test_scalar_stores_equal_the_vector_stores_and_stay_inside_total(eng, cid):
    case = PATHS[cid][0]
    target, reference = _sides(case)
    want = _expected(cid)
    total = len(want)
    rc, n = _plan(eng, target, reference, case.n_chrom)
    assert (rc, n) == (0, total)
    for which, shifts in SHIFTS.items():          # one plan, five fills
        bigs, views = _buffers(total, shifts)
        assert _fill(eng, views, total) == 0, which
        _same(_rows(*views), want, (cid, which))
        assert _sentinels_untouched(bigs, shifts, total), (cid, which)


def test_capacity_refusal_writes_nothing_and_two_fills_are_equal(eng):
    from giql_amd import _lib

    case = PATHS["total-4097"][0]
    target, reference = _sides(case)
    want = _expected("total-4097")
    total = len(want)
    assert _plan(eng, target, reference, 1) == (0, total)
    bigs, views = _buffers(total, (4, 4, 4))
    for cap in (total - 1, 0, -1):
        assert _fill(eng, views, cap) == _lib.GIQL_ERR_CAPACITY, cap
        assert all(bool((b == SENTINEL).all()) for b in bigs), cap
    assert _fill(eng, [None, views[1], views[2]], total) == _lib.GIQL_ERR_INVALID
    assert all(bool((b == SENTINEL).all()) for b in bigs)
    assert _fill(eng, views, total) == 0                      # the plan survived the refusals
    first = _rows(*views)
    _bigs2, views2 = _buffers(total, (4, 4, 4))
    assert _fill(eng, views2, total + 50) == 0                # more room than rows: the rest stays untouched
    _same(first, want, "first fill")
    _same(_rows(*views2), first, "second fill")
    assert _sentinels_untouched(_bigs2, (4, 4, 4), total)


def test_empty_result_fills_with_null_outputs(eng):
    case = R.case_from_counts("no-pieces", [0] * 700, seed=9)
    target, reference = _sides(case)
    assert len(case.expected()) == 0
    assert _plan(eng, target, reference, 1) == (0, 0)
    assert _fill(eng, [None, None, None], 0) == 0
    assert all(int(t.shape[0]) == 0 for t in eng.disjoin(target, reference, 1))


@pytest.mark.parametrize("case", COVERAGE, ids=[c.id for c in COVERAGE])
def test_coverage_logic_against_the_row_by_row_brute_force(eng, case):
    target, reference = _sides(case)
    want = case.expected_row_by_row()
    _same(_rows(*eng.disjoin(target, reference, case.n_chrom)), want, case.id)
    if case.id == "zero-length-reference-rows-cut-never-cover":
        assert len(want) == 0
    if case.id == "book-ended-reference-rows":      # cut at 10 / 20 / 30 and covered throughout: depth stays 1
        assert want.tolist() == [[0, 0, 10], [0, 10, 20], [0, 20, 30], [0, 30, 40], [1, 15, 20], [1, 20, 30]]


# ---------------------------------------------------------------- refusals: documented return codes
def _answers(eng):
    """After a refusal the context answers a valid call correctly."""
    case = COVERAGE[2]
    target, reference = _sides(case)
    _same(_rows(*eng.disjoin(target, reference, case.n_chrom)), case.expected_row_by_row(), "after a refusal")


@pytest.mark.parametrize("bad", [-1, 2])
@pytest.mark.parametrize("where", ["target", "reference", "self"])
def test_chrom_id_outside_the_dictionary(eng, where, bad):
    from giql_amd import _lib

    good = ([0, 1, 1], [0, 10, 30], [20, 40, 50])
    broken = ([0, bad, 1], [0, 10, 30], [20, 40, 50])
    target = _side(good if where == "reference" else broken)
    reference = None if where == "self" else _side(broken if where == "reference" else good)
    rc, n = _plan(eng, target, reference, 2)
    assert rc == _lib.GIQL_ERR_CHROM and n == 0
    outs = [torch.full((8,), SENTINEL, dtype=torch.int32, device=DEV) for _ in range(3)]
    assert _fill(eng, outs, 8) == _lib.GIQL_ERR_STATE           # a failed plan is no plan
    assert all(bool((o == SENTINEL).all()) for o in outs)
    with pytest.raises(_lib.GiqlHipError) as exc:
        eng.disjoin(target, reference, 2)
    assert exc.value.code == _lib.GIQL_ERR_CHROM
    _answers(eng)


def test_rows_without_a_chromosome_dictionary_are_refused(eng):
    from giql_amd import _lib

    some = _side(([0], [0], [9]))
    for reference in (None, some):
        rc, n = _plan(eng, some, reference, 0)
        assert rc == _lib.GIQL_ERR_CHROM and n == 0
        assert _plan(eng, some, reference, -1)[0] == _lib.GIQL_ERR_INVALID
    _answers(eng)


def test_fill_without_a_plan_and_after_a_failed_plan():
    from giql_amd import _lib

    e = _engine({})
    try:
        outs = [torch.full((8,), SENTINEL, dtype=torch.int32, device=DEV) for _ in range(3)]
        assert _fill(e, outs, 8) == _lib.GIQL_ERR_STATE        # a context that has never planned
        assert b"without a successful disjoin_plan" in e._L.giql_hip_last_error()
        good = _side(([0, 0], [0, 10], [20, 30]))
        assert _plan(e, good, None, 1) == (0, 4)
        inverted = _side(([0, 0], [0, 30], [20, 10]))
        assert _plan(e, good, inverted, 1)[0] == _lib.GIQL_ERR_INVALID    # start > end: the plan before it is gone too
        assert _fill(e, outs, 8) == _lib.GIQL_ERR_STATE
        assert all(bool((o == SENTINEL).all()) for o in outs)
        _answers(e)
    finally:
        e.close()


def test_reference_of_more_than_2_29_rows_is_refused_by_its_size(eng):
    """``giql_hip_disjoin_plan_dev_impl`` compares 2 * n with the onesweep limit right after ``check_side`` (which
    reads the struct only) and before ``begin_call``: no buffer is touched, so ``n`` may overstate a tiny one."""
    from giql_amd import _lib

    tiny = _side(([0, 0], [0, 10], [20, 30]))
    huge = tiny.c_struct()
    huge.n = (1 << 29) + 1
    rc, n = _plan(eng, tiny, huge, 1)
    assert rc == _lib.GIQL_ERR_INVALID and b"2^29" in eng._L.giql_hip_last_error()
    rc, n = _plan(eng, huge, None, 1)            # self mode: the target is the reference
    assert rc == _lib.GIQL_ERR_INVALID and b"2^29" in eng._L.giql_hip_last_error()
    _answers(eng)


# ---------------------------------------------------------------- the event sort under every form
LOCAL = {"GIQL_HIP_LOCAL_MIN_ROWS": "1"}
FORMS = {   # name -> (environment, three-stage sort expected, bucket bits, tile order)
    "default": ({}, False, None, 2),
    "local": (LOCAL, True, 16, 2),
    "local13": ({**LOCAL, "GIQL_HIP_LOCAL_BITS": "13"}, True, 13, 2),
    "local14": ({**LOCAL, "GIQL_HIP_LOCAL_BITS": "14"}, True, 14, 2),
    "local15": ({**LOCAL, "GIQL_HIP_LOCAL_BITS": "15"}, True, 15, 2),
    "no_local": ({**LOCAL, "GIQL_HIP_NO_LOCAL_SORT": "1"}, False, None, 2),
    "ticket_order": ({**LOCAL, "GIQL_HIP_LOCAL_BITS": "13", "GIQL_HIP_OS_ORDER": "0"}, True, 13, 0),
    "variant3": ({**LOCAL, "GIQL_HIP_OS_VARIANT": "3"}, False, None, 2),
    "help_at_once": ({**LOCAL, "GIQL_HIP_OS_HELP_AFTER": "0"}, True, 16, 2),
    "injected_timeout": ({"GIQL_HIP_INJECT_TIMEOUT": "1"}, False, None, 0),
}
OS_TILE = 8192          # events per onesweep tile (1,024 threads x 8: os_pass_stride, giql_hip.hip)
TOP = 2**32 - 1


def _table(r, n, span, max_len, n_chrom=1, lo=0):
    c = r.integers(0, n_chrom, n)
    s = lo + r.integers(0, span, n)
    ln = r.integers(1, max_len, n)
    ln[r.random(n) < 0.03] = 0
    return c.astype(np.int64), s.astype(np.int64), (s + ln).astype(np.int64)


@functools.lru_cache(maxsize=None)
def sort_cases():
    """id -> (reference table, target table, n_chrom): the reference is also run alone, in self mode."""
    r = np.random.default_rng(4242)
    out = {}
    for n in (1, 2, OS_TILE // 2 - 1, OS_TILE // 2, OS_TILE // 2 + 1, 3_000, 40_000):
        span = max(100 * n, 1000)
        out[f"rows-{n}"] = (_table(r, n, span, 400), _table(r, 2_000, span, 900), 1)
    # one event alone in its bucket (at every bucket width) between an empty bucket and crowded ones
    c, s, e = _table(r, 3_000, 60_000, 300)
    s, e = np.concatenate([s, [65_536 + 5]]), np.concatenate([e, [3 * 65_536 + 7]])
    out["empty-and-one-row-buckets"] = ((np.zeros(3_001, np.int64), s, e), _table(r, 2_000, 4 * 65_536, 70_000), 1)
    # keys 0 and 0xFFFFFFFE: chromosome 0 over [0, 2^31 - 1], chromosome 1 over [1, 2^31 - 1]
    hi = 2**31 - 1
    c, s, e = _table(r, 3_000, 50_000, 300, 2, lo=1)
    far = r.random(3_000) < 0.5
    s, e = np.where(far, hi - 60_000 + s, s), np.where(far, hi - 60_000 + e, e)
    c[:4], s[:4], e[:4] = [0, 0, 1, 1], [0, hi - 9, 1, hi - 30], [7, hi, 12, hi]
    tc, ts, te = _table(r, 2_000, 50_000, 900, 2, lo=1)
    tfar = r.random(2_000) < 0.5
    ts, te = np.where(tfar, hi - 60_000 + ts, ts), np.where(tfar, hi - 60_000 + te, te)
    out["both-ends-of-the-axis"] = ((c, s, e), (tc, ts, te), 2)
    g = 6_000
    gs = np.arange(g, dtype=np.int64) * 7
    out["gap-free-grid"] = ((np.zeros(g, np.int64), gs[r.permutation(g)], None), _table(r, 2_000, 7 * g, 300), 1)
    grid = out["gap-free-grid"][0]
    out["gap-free-grid"] = ((grid[0], grid[1], grid[1] + 7), out["gap-free-grid"][1], 1)
    s = r.integers(0, 200, 20_000) * 20_000
    out["20000-rows-sharing-200-starts"] = ((np.zeros(20_000, np.int64), s, s + r.integers(1, 3_000, 20_000)),
                                            _table(r, 2_000, 4_000_000, 30_000), 1)
    return out


@functools.lru_cache(maxsize=None)
def sort_expected(cid, mode):
    ref, tgt, _n = sort_cases()[cid]
    return R.brute_force_arrays(*ref) if mode == "self" else R.brute_force_arrays(*tgt, *ref)


def test_sort_cases_are_what_they_claim():
    cases = sort_cases()
    assert 2 * (OS_TILE // 2) == OS_TILE and {f"rows-{n}" for n in (4095, 4096, 4097)} <= set(cases)
    (c, s, e), _t, _n = cases["empty-and-one-row-buckets"]
    for w in (13, 14, 15, 16):
        per = np.bincount(np.concatenate([s, e]) >> w, minlength=(4 << 16) >> w)
        assert per[(65_536 + 5) >> w] == 1 and (per == 0).any() and per.max() > 100, w
    (c, s, e), (tc, ts, te), _n = cases["both-ends-of-the-axis"]
    span = sum(int(max(e[c == k].max(), te[tc == k].max()) - min(s[c == k].min(), ts[tc == k].min()) + 1) for k in (0, 1))
    assert span == TOP and s[c == 0].min() == 0 and e[c == 1].max() == 2**31 - 1     # keys 0 and 0xFFFFFFFE
    (c, s, e), _t, _n = cases["gap-free-grid"]
    assert np.array_equal(np.sort(np.concatenate([s, e]))[1:-1].reshape(-1, 2)[:, 0], np.sort(s)[1:])
    (c, s, e), _t, _n = cases["20000-rows-sharing-200-starts"]
    assert len(np.unique(s)) == 200
    for cid in cases:
        assert len(sort_expected(cid, "self")) > 0 and (cid == "rows-1" or len(sort_expected(cid, "reference")) > 0), cid


@pytest.fixture(scope="module", params=list(FORMS))
def form_eng(request):
    e = _engine(FORMS[request.param][0])
    e.form = request.param
    yield e
    e.close()


def _assert_form(eng):
    _env, local, bits, order = FORMS[eng.form]
    st = eng.stats()
    assert st["sort_local"] == local and not st["sort_resorted"] and st["sort_tile_order"] == order, (eng.form, st)
    if bits is not None:
        assert st["bucket_bits"] == bits, (eng.form, st["bucket_bits"])
    assert st["sort_order_fallbacks"] == (1 if eng.form == "injected_timeout" else 0), (eng.form, st)


@pytest.mark.parametrize("cid", list(sort_cases()))
def test_event_sort_under_every_form(form_eng, cid):
    ref, tgt, n_chrom = sort_cases()[cid]
    d_ref, d_tgt = _side(ref), _side(tgt)
    _same(_rows(*form_eng.disjoin(d_ref, None, n_chrom)), sort_expected(cid, "self"), (form_eng.form, cid, "self"))
    _assert_form(form_eng)
    if cid == "both-ends-of-the-axis":
        assert form_eng.stats()["span"] <= TOP
    _same(_rows(*form_eng.disjoin(d_tgt, d_ref, n_chrom)), sort_expected(cid, "reference"),
          (form_eng.form, cid, "reference"))
    _assert_form(form_eng)
    if cid == "both-ends-of-the-axis":
        assert form_eng.stats()["span"] == TOP


# ---------------------------------------------------------------- more than BS_BIG_MAX events in one bucket
@functools.lru_cache(maxsize=None)
def _oversized_tables():
    from test_context_transitions import BS_BIG_MAX, _oversized

    a, b, _n = _oversized()
    ref = tuple(x.astype(np.int64) for x in (b.chrom, b.start, b.end))
    r = np.random.default_rng(31)
    ts = np.concatenate([r.integers(0, 4_200, 300), r.integers(0, 10_000_000, 200)])
    tgt = (np.zeros(500, np.int64), ts, ts + r.integers(0, 600, 500))
    assert 2 * int((ref[1] < 4000).sum()) > BS_BIG_MAX
    return ref, tgt, (a, b), R.brute_force_arrays(*tgt, *ref), R.brute_force_arrays(*tgt)


def _oversized_round(e, expect_repeat):
    from oracle import pyoracle as ora
    from test_context_transitions import _dev

    ref, tgt, (a, b), want, want_self = _oversized_tables()
    d_ref, d_tgt = _side(ref), _side(tgt)
    _same(_rows(*e.disjoin(d_tgt, d_ref, 1)), want, "the call that meets the oversized bucket")
    st = e.stats()
    assert st["sort_resorted"] == expect_repeat and not st["sort_local"], st
    _same(_rows(*e.disjoin(d_tgt, None, 1)), want_self, "the next DISJOIN")
    _same(_rows(*e.disjoin(d_tgt, d_ref, 1)), want, "the same DISJOIN again")
    ra, rb = e.inner_join(_dev(a), _dev(b), 1)
    assert np.array_equal(ora.sort_pairs(ra.cpu().numpy(), rb.cpu().numpy()), ora.sort_pairs(*ora.c_inner(a, b, "sweep")))
    st = e.stats()
    assert st["sort_resorted"] == expect_repeat and not st["sort_local"], st


def test_oversized_bucket_on_a_fresh_default_context():
    """The default context keeps sides below 2^21 rows in the four global passes, so the 604,100 events of this
    reference never enter the bucket stage there: right rows, no repeat to report."""
    e = _engine({})
    try:
        _oversized_round(e, expect_repeat=False)
    finally:
        e.close()


@pytest.mark.parametrize("env", [LOCAL, {**LOCAL, "GIQL_HIP_LOCAL_BITS": "13"}], ids=["local", "local13"])
def test_oversized_bucket_repeats_the_plan_with_four_passes(env):
    """A fresh context without the 2^21-row floor: the events take the bucket stage, one bucket holds more than
    BS_BIG_MAX of them (GIQL_STATUS_RESORT), DISJOIN's later kernels have run over unsorted events by then, and
    ``with_order_fallback`` repeats the plan with four passes -- for good on this context."""
    e = _engine(env)
    try:
        _oversized_round(e, expect_repeat=True)
    finally:
        e.close()


def test_oversized_bucket_met_on_a_density_context_after_another_calls_span(monkeypatch):
    """The production density rule: the width comes from the previous call's span (a sparse-looking INNER join here),
    under which these events look dense enough for narrow buckets."""
    from test_context_transitions import _density_engine, op_inner_join, Log

    e = _density_engine(monkeypatch)
    try:
        op_inner_join(e, "w16", Log(), "settle", 1)
        assert e.stats()["sort_local"] and not e.stats()["sort_resorted"]
        _oversized_round(e, expect_repeat=True)
    finally:
        e.close()
