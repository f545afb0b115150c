"""The compact plan: ``giql_hip_fill_from_plan_dev`` on hand-built plans, ``giql_hip_inner_plan_export_dev`` from every
plan form, and the multi-rank layout of ``giql_amd.distributed`` on one GPU.

The compact plan -- per query row ``{row id, first match, count}`` plus the other side's row ids in sorted order -- is
what ranks exchange instead of the pairs (``include/giql_hip.h``, "compact plan"; reference semantics: the UNION ALL
over per-chromosome branches, ``src/giql/expanders/_per_chrom.py:46-74``).

A. ``fill_from_plan`` is the one entry point where a test hands ``k_partition`` / ``k_fill``
   (``giql_amd/csrc/join_kernels.hip.h``) arrays of its own making: ``tests/_plans.py`` builds one plan per path of
   ``k_fill`` and says -- on the CPU, without the ``gpu`` marker -- which path each one takes.  The reference is the
   three-line numpy expansion, itself checked against two plain loops.
B. The export is checked against the oracle after plans of every form ``plan_uniform`` has (``giql_hip.hip``): on its
   own (numpy expansion of the exported arrays) and as a round trip (``fill_from_plan``).
C. ``hip_local_plan`` / ``hip_expand`` drive the layout of ``sharded_inner_join_compact`` for ``world`` ranks in one
   process.

Every comparison is exact, on integers.
"""

import ctypes
import os

import numpy as np
import pytest

import _plans as P
from oracle import pyoracle as ora
from test_gpu_parity import dev, rand_side, uniform_side

torch = pytest.importorskip("torch")

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -77_777_777      # no id of any plan or table here
PAD = 100
CASES = P.plan_cases()
CONTEXTS = {"default": {}, "narrow": {"GIQL_HIP_LOCAL_MIN_ROWS": "1", "GIQL_HIP_LOCAL_BITS": "13"}}


def _engine(env=None):
    """A context created under the switches ``env`` (read once, at creation: ``giql_hip.hip`` ``read_switches``)."""
    from giql_amd.engine import HipEngine

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    with pytest.MonkeyPatch.context() as mp:
        for k, v in (env or {}).items():
            mp.setenv(k, v)
        return HipEngine(0)


@pytest.fixture(scope="module", params=list(CONTEXTS))
def eng(request):
    e = _engine(CONTEXTS[request.param])
    yield e
    e.close()


def _full(n, value=SENT):
    return torch.full((int(n),), value, dtype=torch.int32, device="cuda:0")


def _up(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.int32)).to("cuda:0")


# ===================================================================== A. on the CPU: the reference and the cases
def test_numpy_expansion_equals_two_plain_loops():
    r = np.random.default_rng(5)
    plans = [P.build_plan(1, [0, 3, 0, 0, 2, 1], n_s=9), P.build_plan(2, [4], n_s=4), P.build_plan(3, [0, 0], n_s=3),
             P.build_plan(4, r.integers(0, 6, 300), n_s=40, lo=r.integers(0, 35, 300)),
             P.build_plan(5, r.integers(0, 4, 50), n_s=20, q_rid=r.integers(0, 5, 50), q_add=0, s_add=-10)]
    for q_rid, lo, cnt, s_rid in plans:
        row_q, row_s = P.expand_np(q_rid, lo, cnt, s_rid)
        want_q, want_s = P.expand_loops(q_rid, lo, cnt, s_rid)
        assert row_q.tolist() == want_q and row_s.tolist() == want_s
        assert len(want_q) == int(cnt.sum())
        tq, ts = P._np_expand(*(torch.from_numpy(x) for x in (q_rid, lo, cnt, s_rid)), len(want_q))
        assert tq.tolist() == want_q and ts.tolist() == want_s
    # by hand: rows 7 and 9 with two and one matches
    row_q, row_s = P.expand_np([7, 8, 9], [2, 0, 0], [2, 0, 1], [50, 51, 52, 53])
    assert row_q.tolist() == [7, 7, 9] and row_s.tolist() == [52, 53, 50]
    assert P.pair_words([-1, 0], [5, -2]).tolist() == [(0 << 32) | 0xFFFFFFFE, (0xFFFFFFFF << 32) | 5]


def test_every_case_reaches_the_path_it_is_named_for():
    """The cases of tests/_plans.py against the numpy mirror of k_partition / k_fill: whoever retunes FILL_NT,
    GIQL_FILL_ITEMS or FILL_QCAP is told here to redesign them."""
    src = open(os.path.join(ROOT, "giql_amd", "csrc", "join_kernels.hip.h")).read()
    assert "#define GIQL_FILL_NT 1024" in src and "constexpr int FILL_QCAP = 4 * FILL_NT;" in src
    assert "#define GIQL_FILL_ITEMS 16" in open(os.path.join(ROOT, "giql_amd", "csrc", "giql_hip.hip")).read()
    assert "constexpr int SCAN_TILE = SCAN_NT * SCAN_ITEMS;  // 4096" in open(
        os.path.join(ROOT, "giql_amd", "csrc", "scan.hip.h")).read()
    reached = set()
    cl = {}
    for name, (q_rid, lo, cnt, s_rid) in CASES.items():
        assert bool(np.all(lo.astype(np.int64) + cnt <= s_rid.shape[0])) and int(lo.min()) >= 0, name
        assert q_rid.shape == lo.shape == cnt.shape and int(cnt.sum()) <= 5_000_000, name
        cl[name] = c = P.classify(cnt)
        reached |= c["paths"]
        if name in P.EXPECT:
            assert P.EXPECT[name] in c["paths"], (name, c["paths"])
    assert reached == set(P.PATHS)
    wp = {name: np.asarray(c["win_path"]) for name, c in cl.items()}
    for name in ("tiny_1", "tiny_2", "tiny_63", "tiny_64", "tiny_65"):
        assert cl[name]["n_tiles"] == 1 and cl[name]["total"] < 4 * P.WINDOW
    assert set(wp["long_rows"]) == {"few"} and int(cl["long_rows"]["win_starts"].max()) <= 4
    assert np.mean(wp["medium_rows"] == "mask") > 0.9 and not cl["medium_rows"]["win_dup"].any()
    c = cl["bursts"]
    assert int(c["win_starts"].max()) == P.WINDOW and not c["win_dup"].any() and int(c["tile_rows"].max()) < P.FILL_QCAP
    assert np.sum(wp["bursts"] == "slow") >= 10
    c = cl["empty_among_full"]
    assert np.sum((wp["empty_among_full"] == "slow") & c["win_dup"]) > 1000 and int(c["win_starts"].max()) < P.WINDOW
    c = cl["empty_runs"]
    assert set(c["tile_path"]) == {"search"} and int(c["tile_rows"].min()) > P.FILL_QCAP and c["n_tiles"] >= 7
    c = cl["all_ones"]                                     # 16,385 rows in a full tile; the 17 pairs left over are staged
    assert c["tile_path"] == ["search"] * 3 + ["staged"] and c["tile_rows"].tolist() == [P.TILE + 1] * 3 + [17]
    c = cl["giant_row"]
    assert np.sum(c["tile_rows"] == 1) >= 4 and set(c["tile_path"]) == {"staged"}      # tiles wholly inside the row
    for name, nt, partial in (("total_tile", 1, False), ("total_tile_minus_1", 1, True),
                              ("total_tile_plus_1", 2, True), ("total_two_tiles", 2, False)):
        assert cl[name]["n_tiles"] == nt and bool(cl[name]["tile_partial"].any()) == partial, name
    cnt = CASES["row_ends_on_tile_then_empty"][2]
    off = np.cumsum(cnt)
    k = int(np.searchsorted(off, P.TILE, "left"))
    assert off[k] == P.TILE and cnt[k] > 0 and cnt[k + 1] == 0 and off[-1] > P.TILE
    for n_q in (4095, 4096, 4097, 8193):
        assert CASES[f"scan_{n_q}"][0].shape[0] == n_q
    ids = CASES["negative_ids"]
    assert int(ids[0].max()) < 0 and int(ids[3].min()) < 0 < int(ids[3].max())
    assert np.unique(CASES["repeated_q_rid"][0]).shape[0] <= 100
    assert np.unique(CASES["same_lo"][1]).shape[0] == 1 and bool(np.all(np.diff(CASES["descending_lo"][1]) <= 0))


def test_classifier_on_plans_small_enough_to_read():
    c = P.classify([0] * 10)
    assert c["total"] == 0 and c["paths"] == set()
    c = P.classify([64] * 256)                      # one full tile, one start per window (a wave's first: none)
    assert c["n_tiles"] == 1 and c["paths"] == {"few"} and int(c["win_starts"].max()) == 1
    assert c["win_starts"][0] == 0 and c["win_starts"][16] == 0 and c["tile_rows"].tolist() == [256]
    c = P.classify([1] * 100)                       # 63 / 36 starts, a partial tile
    assert c["win_starts"].tolist() == [63, 36] and c["win_path"] == ["mask", "mask"] and "partial" in c["paths"]
    c = P.classify([1] * 64 + [0, 0] + [1] * 10)    # window 1: three rows share the start 64
    assert c["win_starts"].tolist() == [63, 12] and c["win_dup"].tolist() == [False, True]
    assert c["win_path"] == ["mask", "slow"]
    c = P.classify([100] + [1] * 70)                # starts 100..169: window 2 = [128, 192) holds 42 of them
    assert c["win_starts"].tolist() == [0, 28, 42]
    c = P.classify([60] + [1] * 80)                 # starts 60..139: window 1 = [64, 128) holds 64 of them
    assert c["win_starts"].tolist() == [4, 64, 12] and c["win_path"] == ["few", "slow", "mask"]
    c = P.classify([0] * 5000 + [P.TILE])           # leading empty rows belong to no tile: part[0] is the last of them
    assert c["tile_rows"].tolist() == [1] and c["paths"] == {"few"}
    c = P.classify([P.TILE] + [0] * 5000 + [1])     # 5,002 rows start at or before the first tile's end
    assert c["tile_rows"].tolist() == [5002, 1] and c["tile_path"] == ["search", "staged"]
    assert c["paths"] == {"search", "few", "partial"}


# ===================================================================== A. on the GPU
class _DevPlan:
    """A case on the device, with its reference."""

    def __init__(self, arrays):
        q_rid, lo, cnt, s_rid = arrays
        assert bool(np.all(lo.astype(np.int64) + cnt <= s_rid.shape[0]))      # never feed the GPU anything else
        self.dev = tuple(_up(x) for x in arrays)
        self.want_q, self.want_s = P.expand_np(*arrays)
        self.n = int(self.want_q.shape[0])
        self.words = P.pair_words(self.want_q, self.want_s)


def _fill_and_check(e, plan, expected, pad):
    rq, rs = _full(plan.n + pad), _full(plan.n + pad)
    got = e.fill_from_plan(*plan.dev, rq, rs, n_pairs_expected=plan.n if expected else -1)
    assert got == plan.n
    gq, gs = rq.cpu().numpy(), rs.cpu().numpy()
    n = plan.n
    assert np.array_equal(P.pair_words(gq[:n], gs[:n]), plan.words)            # the multiset the header promises
    assert np.array_equal(gq[:n], plan.want_q) and np.array_equal(gs[:n], plan.want_s)    # pair k of row i at off[i] + k
    assert bool((gq[n:] == SENT).all()) and bool((gs[n:] == SENT).all())


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_fill_from_plan_equals_the_numpy_expansion(eng, name):
    """Entry i of the output is entry i of the reference (and so the sorted pairs are equal too): pair k of query row
    i lies at off[i] + k in every path of k_fill, the binary-search fallback included."""
    plan = _DevPlan(CASES[name])
    for expected in (False, True):
        for pad in (0, PAD):
            _fill_and_check(eng, plan, expected, pad)


@gpu
def test_fill_from_plan_scratch_grows_and_shrinks_on_one_context(eng):
    plans = {k: _DevPlan(CASES[k]) for k in ("tiny_2", "scan_4097", "medium_rows", "empty_runs", "giant_row", "tiny_65")}
    empty = _DevPlan(P.build_plan(7, np.zeros(100, np.int64)))
    assert empty.n == 0
    for k in ("tiny_2", "scan_4097", "medium_rows", "empty_runs", "tiny_65", "giant_row", "tiny_2", "medium_rows"):
        _fill_and_check(eng, plans[k], True, PAD)
        _fill_and_check(eng, empty, False, PAD)
        _fill_and_check(eng, plans[k], False, 0)
    _fill_and_check(eng, empty, True, 0)


@gpu
def test_fill_from_plan_never_writes_at_or_past_capacity(eng):
    """``include/giql_hip.h``: "a wrong expectation cannot overrun `capacity`".  The outputs are the first ``cap``
    entries of a larger allocation full of a sentinel, so a write past ``cap`` lands in memory the test owns.

    What the call returns today when the expectation is too LOW (``T - 2 TILE``), or when it fits a capacity that
    the true count does not: GIQL_OK and the caller's own number as ``*n_pairs`` -- in the first case a prefix of
    the pairs is written, in the second nothing.  Only the promise is asserted for those."""
    from giql_amd import _lib

    plan = _DevPlan(CASES["medium_rows"])
    T, TILE = plan.n, P.TILE
    assert T > 8 * TILE

    def run(cap, expected):
        rq, rs = _full(cap + 4 * TILE), _full(cap + 4 * TILE)
        code, got = _lib.GIQL_OK, None
        try:
            got = eng.fill_from_plan(*plan.dev, rq[:cap], rs[:cap], n_pairs_expected=expected)
        except _lib.GiqlHipError as exc:
            code = exc.code
        torch.cuda.synchronize()
        return code, got, rq.cpu().numpy(), rs.cpu().numpy()

    for cap in (T - 1, T // 2, 1):               # too small, and the call knows: an error, nothing written
        code, _, gq, gs = run(cap, -1)
        assert code == _lib.GIQL_ERR_CAPACITY
        assert bool((gq == SENT).all()) and bool((gs == SENT).all())
    for cap in (T + 3 * TILE, T + 3 * TILE + 5):  # the caller expects more than there is
        code, _, gq, gs = run(cap, T + 3 * TILE)
        assert code == _lib.GIQL_OK
        assert np.array_equal(gq[:T], plan.want_q) and np.array_equal(gs[:T], plan.want_s)
        assert bool((gq[T:] == SENT).all()) and bool((gs[T:] == SENT).all())
    for cap in (T, T + 50):                        # ... less than there is
        code, got, gq, gs = run(cap, T - 2 * TILE)
        print(f"[capacity] expected T - 2 TILE, capacity {cap - T:+d}: rc {code}, n_pairs {got} (T = {T})")
        assert bool((gq[cap:] == SENT).all()) and bool((gs[cap:] == SENT).all())
    for cap, expected in ((T - TILE, T - 3 * TILE), (T - 1, T - 1), (T - TILE - 7, 0)):   # ... and buffers to match
        code, got, gq, gs = run(cap, expected)
        print(f"[capacity] expected {expected - T:+d}, capacity {cap - T:+d}: rc {code}, n_pairs {got} (T = {T})")
        assert bool((gq[cap:] == SENT).all()) and bool((gs[cap:] == SENT).all())
    _fill_and_check(eng, plan, True, PAD)          # the context is none the worse for it


# ===================================================================== B. export from every plan form
class _Want:
    """The oracle's answer for one pair of tables."""

    def __init__(self, a, b):
        self.a, self.b = a, b
        ra, rb = ora.c_inner(a, b, "sweep")
        self.n = int(ra.shape[0])
        self.words = P.pair_words(ra, rb)
        self.count = {"a": np.bincount(ra, minlength=a.n), "b": np.bincount(rb, minlength=b.n)}
        assert np.array_equal(self.count["a"], ora.c_count(a, b, "sweep"))
        self.da, self.db = dev(a), dev(b)

    def query(self):
        """The query side of the compact form: the side of free length; of two fixed-length sides, the plan's A --
        the smaller table (``giql_hip.hip`` ``decide_form``; the larger side is planned as B)."""
        fixed = [s.n > 0 and np.unique(s.end.astype(np.int64) - s.start).shape[0] == 1 for s in (self.a, self.b)]
        if fixed[0] != fixed[1]:
            return "b" if fixed[0] else "a"
        assert fixed[0], "no compact form: both sides of free length"
        return "b" if self.a.n > self.b.n else "a"


def _export_raw(e, bufs, q_capacity, s_capacity, adds=(0, 0)):
    """The C-ABI call itself: ``(rc, query_is_a, n_q, n_s)`` -- the sizes are reported with GIQL_ERR_CAPACITY too."""
    qa, nq, ns = ctypes.c_int32(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
    ptr = [None if b is None else e._dev_ptr(b, "buffer", torch.int32) for b in bufs]
    rc = e._L.giql_hip_inner_plan_export_dev(e._h, *ptr, int(q_capacity), int(s_capacity), int(adds[0]), int(adds[1]),
                                             ctypes.byref(qa), ctypes.byref(nq), ctypes.byref(ns), e._stream())
    return rc, qa.value, nq.value, ns.value


def _check_export(e, w, n, adds, filler=None):
    """The plan the context ``e`` holds for ``w``'s tables, exported with the id offsets ``adds`` = (A, B)."""
    a, b = w.a, w.b
    query = w.query()
    q_is_a, n_q, n_s = e.plan_sizes()
    assert (q_is_a, n_q, n_s) == ((query == "a"), (a.n, b.n)[query == "b"], (b.n, a.n)[query == "b"])
    assert n == w.n
    bufs = [_full(n_q + PAD), _full(n_q + PAD), _full(n_q + PAD), _full(n_s + PAD)]
    assert e.plan_export(*bufs, rid_add_a=adds[0], rid_add_b=adds[1]) == (q_is_a, n_q, n_s)
    again = [_full(n_q + PAD), _full(n_q + PAD), _full(n_q + PAD), _full(n_s + PAD)]
    assert e.plan_export(*again, rid_add_a=adds[0], rid_add_b=adds[1]) == (q_is_a, n_q, n_s)
    assert all(torch.equal(x, y) for x, y in zip(bufs, again))                  # exporting twice: identical arrays
    q_rid, lo, cnt, s_rid = (x.cpu().numpy() for x in bufs)
    for x, m in ((q_rid, n_q), (lo, n_q), (cnt, n_q), (s_rid, n_s)):
        assert bool((x[m:] == SENT).all())
    q_rid, lo, cnt, s_rid = q_rid[:n_q], lo[:n_q].astype(np.int64), cnt[:n_q].astype(np.int64), s_rid[:n_s]
    q_add, s_add = (adds[0], adds[1]) if q_is_a else (adds[1], adds[0])         # each side's own offset
    assert np.array_equal(np.sort(q_rid.astype(np.int64) - q_add), np.arange(n_q))
    assert np.array_equal(np.sort(s_rid.astype(np.int64) - s_add), np.arange(n_s))
    assert int(lo.min()) >= 0 and int(cnt.min()) >= 0 and bool(np.all(lo + cnt <= n_s))
    assert np.array_equal(cnt, w.count[query][q_rid.astype(np.int64) - q_add])
    assert int(cnt.sum()) == n
    eq, es = P.expand_np(q_rid, lo, cnt, s_rid)                                 # the export on its own
    lq, ls = eq.astype(np.int64) - q_add, es.astype(np.int64) - s_add
    assert np.array_equal(P.pair_words(*((lq, ls) if q_is_a else (ls, lq))), w.words)
    f = filler or e                                                             # ... and the round trip
    rq, rs = _full(n + PAD), _full(n + PAD)
    assert f.fill_from_plan(bufs[0][:n_q], bufs[1][:n_q], bufs[2][:n_q], bufs[3][:n_s], rq, rs, n_pairs_expected=n) == n
    gq, gs = rq.cpu().numpy(), rs.cpu().numpy()
    assert np.array_equal(gq[:n], eq) and np.array_equal(gs[:n], es)
    assert bool((gq[n:] == SENT).all()) and bool((gs[n:] == SENT).all())


def _plan_and_check(e, w, n_chrom, adds=(1000, 50), filler=None):
    n = e.inner_plan(w.da, w.db, n_chrom)
    st = e.stats()
    print(f"[export] {w.a.n} x {w.b.n}: "
          + ", ".join(f"{k}={st[k]}" for k in ("join_form", "swapped", "sort_local", "count_fused", "span_hist",
                                                "bucket_bits", "sort_resorted", "presorted")))
    _check_export(e, w, n, adds, filler)
    assert st["swapped"] == (w.a.n > w.b.n) and (st["n_a"], st["n_b"]) == (w.a.n, w.b.n)
    assert st["join_form"] == ("uniform_b" if w.query() == "a" else "uniform_a")
    return st


def _three(e, w, n_chrom, adds=(1000, 50), **flags):
    """Three plans in a row (the second and third run on the context's guesses), each of the form ``flags`` names."""
    for k in range(3):
        st = _plan_and_check(e, w, n_chrom, adds if k != 1 else (adds[1], adds[0] + 3))
        for name, value in flags.items():
            assert st[name] == value, (k, name, st)
    return st


def _peaks_reads(seed=3100, n_peaks=20_000, n_reads=300_000, n_chrom=6, span=30_000_000):
    return rand_side(seed, n_peaks, n_chrom, span, 900), uniform_side(seed + 1, n_reads, n_chrom, span, 150)


@gpu
def test_export_default_context_both_orders_and_two_fixed_lengths():
    peaks, reads = _peaks_reads()
    short = uniform_side(3103, 40_000, 6, 30_000_000, 75)
    e = _engine()
    try:
        plain = dict(sort_local=False, count_fused=False, sort_resorted=False, presorted=False)
        st = _three(e, _Want(peaks, reads), 6, span_hist=True, **plain)
        assert st["join_form"] == "uniform_b" and not st["swapped"]
        st = _three(e, _Want(reads, peaks), 6, span_hist=True, **plain)           # the larger table first
        assert st["join_form"] == "uniform_a" and st["swapped"]
        st = _three(e, _Want(short, reads), 6, **plain)                           # both of fixed length
        assert st["join_form"] == "uniform_b" and not st["swapped"]
        st = _three(e, _Want(reads, short), 6, **plain)
        assert st["join_form"] == "uniform_a" and st["swapped"]
        st = _three(e, _Want(reads, rand_side(3104, 400_000, 6, 30_000_000, 900)), 6, span_hist=False, **plain)
        assert st["join_form"] == "uniform_a" and not st["swapped"]               # the fixed-length side the smaller one
    finally:
        e.close()


@gpu
@pytest.mark.parametrize("fuse", [True, False], ids=["fused_count", "count_kernel"])
def test_export_three_stage_sort_both_orders(fuse):
    env = {"GIQL_HIP_LOCAL_MIN_ROWS": "1"}
    if not fuse:
        env["GIQL_HIP_NO_FUSE_COUNT"] = "1"
    peaks, reads = _peaks_reads(3110, 60_000, 900_000)
    e = _engine(env)
    try:
        form = dict(sort_local=True, count_fused=fuse, bucket_bits=16, sort_resorted=False, presorted=False, span_hist=True)
        st = _three(e, _Want(peaks, reads), 6, **form)
        assert st["join_form"] == "uniform_b" and not st["swapped"]
        st = _three(e, _Want(reads, peaks), 6, **form)
        assert st["join_form"] == "uniform_a" and st["swapped"]
    finally:
        e.close()


@gpu
@pytest.mark.parametrize("bits", [13, 14, 15])
def test_export_narrow_buckets(bits):
    peaks, reads = _peaks_reads(3120 + bits, 30_000, 500_000, 5, 20_000_000)
    e = _engine({"GIQL_HIP_LOCAL_MIN_ROWS": "1", "GIQL_HIP_LOCAL_BITS": str(bits)})
    try:
        form = dict(sort_local=True, count_fused=True, bucket_bits=bits, sort_resorted=False)
        _three(e, _Want(peaks, reads), 5, **form)
        assert _three(e, _Want(reads, peaks), 5, **form)["swapped"]
    finally:
        e.close()


@gpu
def test_export_without_three_stage_sort_and_raw_column_sorts():
    peaks, reads = _peaks_reads(3130)
    e = _engine({"GIQL_HIP_NO_LOCAL_SORT": "1", "GIQL_HIP_NO_SPAN_HIST": "1"})
    try:
        form = dict(sort_local=False, count_fused=False, span_hist=False, sort_resorted=False)
        _three(e, _Want(peaks, reads), 6, **form)
        assert _three(e, _Want(reads, peaks), 6, **form)["swapped"]
    finally:
        e.close()


@gpu
def test_classic_sort_plans_in_the_general_form_and_export_says_so():
    """GIQL_HIP_SORT=classic (with the two switches above) never decides a fixed-length form (``begin_attempt`` reads
    the lengths back only on the one-sweep path), so its plan has no compact form: the export answers GIQL_ERR_STATE,
    ``hip_local_plan`` returns None, and the pairs are exchanged instead."""
    from giql_amd import _lib
    from giql_amd import distributed as D

    peaks, reads = _peaks_reads(3130)
    w = _Want(peaks, reads)
    e = _engine({"GIQL_HIP_NO_LOCAL_SORT": "1", "GIQL_HIP_NO_SPAN_HIST": "1", "GIQL_HIP_SORT": "classic"})
    try:
        for _ in range(3):
            n = e.inner_plan(w.da, w.db, 6)
            st = e.stats()
            assert n == w.n and st["join_form"] == "general" and not st["sort_local"] and not st["span_hist"]
            bufs = [_full(peaks.n), _full(peaks.n), _full(peaks.n), _full(reads.n)]
            with pytest.raises(_lib.GiqlHipError) as exc:
                e.plan_export(*bufs)
            assert exc.value.code == _lib.GIQL_ERR_STATE
            assert all(bool((x == SENT).all()) for x in bufs)
            ra, rb = _full(n), _full(n)
            e.inner_fill(ra, rb)                    # the refused export leaves the plan as it was
            assert np.array_equal(P.pair_words(ra.cpu().numpy(), rb.cpu().numpy()), w.words)
        plan = D.hip_local_plan(e)(peaks.chrom, peaks.start, peaks.end, (0, 0), reads.chrom, reads.start, reads.end,
                                   (0, 0), 6)
        assert plan is None
    finally:
        e.close()


@gpu
def test_export_after_the_four_pass_fallback(monkeypatch):
    from test_context_transitions import _density_engine, _oversized

    a, b, nch = _oversized()
    peaks, reads = _peaks_reads(3140)
    e = _density_engine(monkeypatch)
    try:
        _three(e, _Want(peaks, reads), 6, sort_resorted=False)
        w = _Want(a, b)
        for k in range(3):
            st = _plan_and_check(e, w, nch)
        assert st["sort_resorted"] and not st["sort_local"] and st["join_form"] == "uniform_b"
        st = _three(e, _Want(peaks, reads), 6, sort_local=False, sort_resorted=True)     # for good
        assert _three(e, _Want(reads, peaks), 6, sort_local=False, sort_resorted=True)["swapped"]
    finally:
        e.close()


def _sorted_side(side):
    order = np.lexsort((side.start, side.chrom))
    return ora.Side(side.chrom[order], side.start[order], side.end[order], side.start_off, side.end_off)


@gpu
@pytest.mark.parametrize("local", [False, True], ids=["one_sweep", "three_stage"])
@pytest.mark.parametrize("which", ["fixed", "query", "both"])
def test_export_of_sides_that_arrived_sorted(which, local):
    """A side that skipped its sort has its row ids written by k_iota / k_keygen_stream, not by a sort."""
    a = rand_side(3151, 60_000, 7, 5_000_000, 900)
    b = uniform_side(3152, 250_000, 7, 5_000_000, 150)
    sa = _sorted_side(a) if which in ("query", "both") else a
    sb = _sorted_side(b) if which in ("fixed", "both") else b
    e = _engine({"GIQL_HIP_LOCAL_MIN_ROWS": "1"} if local else {})
    try:
        # (a side that skipped its sort reports no sort form: the fused count tells the two contexts apart)
        _three(e, _Want(sa, sb), 7, presorted=True, count_fused=local)
        assert _three(e, _Want(sb, sa), 7, presorted=True, count_fused=local)["swapped"]
        w = _Want(a, b)                           # the same context meets the shuffled tables
        _plan_and_check(e, w, 7)
        st = _plan_and_check(e, w, 7)
        assert not st["presorted"]
    finally:
        e.close()


@gpu
def test_export_all_encoding_pairs():
    r = np.random.default_rng(3160)
    e = _engine()
    try:
        for i, enc_a in enumerate(ora.ENCODING_OFFSETS):
            for j, enc_b in enumerate(ora.ENCODING_OFFSETS):
                a = rand_side(3161 + i, 5_000, 4, 2_000_000, 700, enc=enc_a)
                st = r.integers(0, 2_000_000, 50_000).astype(np.int32)
                so, eo = ora.ENCODING_OFFSETS[enc_b]
                b = ora.Side(r.integers(0, 4, st.size).astype(np.int32), st, st + np.int32(120), so, eo)
                w = _Want(a, b)
                assert w.n > 5_000
                _plan_and_check(e, w, 4, adds=(10 * i + 1, 1000 * j + 7))
                if i == j:
                    assert _plan_and_check(e, _Want(b, a), 4, adds=(3, 900_000))["swapped"]
    finally:
        e.close()


@gpu
@pytest.mark.parametrize("ctx", list(CONTEXTS) + ["local"])
def test_export_edges(ctx):
    env = {"local": {"GIQL_HIP_LOCAL_MIN_ROWS": "1"}, **CONTEXTS}[ctx]
    r = np.random.default_rng(3170)
    e = _engine(env)
    try:
        reads = uniform_side(3171, 200_000, 6, 3_000_000, 150)
        # most query rows match nothing
        far = rand_side(3172, 30_000, 6, 300_000_000, 400)
        w = _Want(far, reads)
        assert np.mean(w.count["a"] == 0) > 0.9 and w.n > 1000
        _three(e, w, 6)
        # one chromosome on the query side only, another on the fixed-length side only
        q7 = rand_side(3173, 20_000, 7, 3_000_000, 600)
        q7.chrom[q7.chrom == 2] = 6
        w = _Want(q7, reads)
        assert w.count["a"][q7.chrom == 6].sum() == 0 and w.count["b"][reads.chrom == 2].sum() == 0
        _three(e, w, 7)
        assert _plan_and_check(e, _Want(reads, q7), 7)["swapped"]
        # one chromosome; 1,025 of them
        _three(e, _Want(rand_side(3174, 10_000, 1, 4_000_000, 900), uniform_side(3175, 150_000, 1, 4_000_000, 200)), 1)
        _three(e, _Want(rand_side(3176, 20_000, 1025, 1_000_000, 900), uniform_side(3177, 300_000, 1025, 1_000_000, 200)),
               1025, span_hist=False)
        # fixed length 1
        w = _Want(rand_side(3178, 20_000, 3, 600_000, 500), uniform_side(3179, 100_000, 3, 600_000, 1))
        assert w.n > 100_000
        _three(e, w, 3)
        # a query row too long for the fused count's windows, on a context that has fused before
        peaks, reads = _peaks_reads(3180)
        st = _three(e, _Want(peaks, reads), 6)
        fused = st["count_fused"]
        assert fused == (ctx != "default")
        long_peaks = ora.Side(peaks.chrom.copy(), peaks.start.copy(), peaks.end.copy())
        k = int(r.integers(0, peaks.n))
        long_peaks.end[k] = long_peaks.start[k] + 70_000
        st = _three(e, _Want(long_peaks, reads), 6, count_fused=False)
        assert _three(e, _Want(peaks, reads), 6)["count_fused"] == fused
    finally:
        e.close()


@gpu
def test_export_contract_short_buffers_empty_plan_and_a_plan_kept_by_a_refused_join(eng):
    from giql_amd import _lib

    peaks, reads = _peaks_reads(3190, 8_000, 120_000)
    w = _Want(peaks, reads)
    n = eng.inner_plan(w.da, w.db, 6)
    bufs = [_full(peaks.n), _full(peaks.n), _full(peaks.n), _full(reads.n)]
    for qcap, scap in ((peaks.n - 1, reads.n), (peaks.n, reads.n - 1), (0, 0)):
        rc, qa, nq, ns = _export_raw(eng, bufs, qcap, scap, (5, 6))
        assert (rc, qa, nq, ns) == (_lib.GIQL_ERR_CAPACITY, 1, peaks.n, reads.n)
        assert all(bool((x == SENT).all()) for x in bufs)
    rc, qa, nq, ns = _export_raw(eng, [None] * 4, 0, 0)
    assert (rc, qa, nq, ns) == (_lib.GIQL_ERR_CAPACITY, 1, peaks.n, reads.n)
    _check_export(eng, w, n, (5, 6))                          # still exportable
    # a plan without pairs
    other = ora.Side(reads.chrom + np.int32(6), reads.start, reads.end)
    assert eng.inner_plan(w.da, dev(other), 12) == 0
    one = [_full(1) for _ in range(4)]
    assert _export_raw(eng, one, 1, 1)[0::2] == (_lib.GIQL_OK, 0) and _export_raw(eng, one, 1, 1)[3] == 0
    assert _export_raw(eng, [None] * 4, 0, 0)[0] == _lib.GIQL_OK
    assert eng.plan_sizes()[1:] == (0, 0) and all(int(x[0]) == SENT for x in one)
    # inner_join_into with buffers too small: GIQL_ERR_CAPACITY, "the plan stays valid"
    for k in range(3):
        ra, rb = _full(w.n // 2), _full(w.n // 2)
        with pytest.raises(_lib.GiqlHipError) as exc:
            eng.inner_join_into(w.da, w.db, 6, ra, rb)
        assert exc.value.code == _lib.GIQL_ERR_CAPACITY and eng.last_pairs == w.n
        _check_export(eng, w, eng.last_pairs, (70 + k, 9_000))
        ra, rb = _full(w.n + PAD), _full(w.n + PAD)          # ... and with buffers that hold them
        assert eng.inner_join_into(w.da, w.db, 6, ra, rb) == w.n
        assert np.array_equal(P.pair_words(ra[:w.n].cpu().numpy(), rb[:w.n].cpu().numpy()), w.words)


# ===================================================================== C. the multi-rank layout on one GPU
@pytest.fixture(scope="module")
def two_engines():
    plan_eng, fill_eng = _engine(), _engine()      # a receiver is another context
    yield plan_eng, fill_eng
    plan_eng.close()
    fill_eng.close()


def _ranks(engines, a, b, n_chrom, world, none_on=()):
    """Lines 396-426 of ``sharded_inner_join_compact`` for every rank in turn, without the collectives."""
    from giql_amd import distributed as D

    local_plan, expand = D.hip_local_plan(engines[0]), D.hip_expand(engines[1])
    (ca, sa, ea), (cb, sb, eb) = a, b
    blocks = []
    for rank in range(world):
        ia, ib = D.unit_rows(ca, cb, n_chrom, world, rank)
        plan = local_plan(ca[ia], sa[ia], ea[ia], (0, 0), cb[ib], sb[ib], eb[ib], (0, 0), n_chrom)
        if rank in none_on:
            assert plan is None
            continue
        assert plan is not None
        q_is_a, q_rid, lo, cnt, s_rid, n_pairs = plan
        assert q_rid.shape == lo.shape == cnt.shape and int(cnt.sum()) == n_pairs
        map_q, map_s = (ia, ib) if q_is_a else (ib, ia)
        blocks.append((q_is_a, _up(map_q)[q_rid.long()], lo, cnt, _up(map_s)[s_rid.long()], n_pairs))
    return _expand_blocks(expand, blocks)


def _expand_blocks(expand, blocks):
    out_a, out_b = [np.zeros(0, np.int32)], [np.zeros(0, np.int32)]
    for q_is_a, q_rid, lo, cnt, s_rid, n_pairs in blocks:
        if n_pairs == 0:
            continue
        row_q, row_s = expand(q_rid, lo, cnt, s_rid, n_pairs)
        assert row_q.shape[0] == n_pairs == row_s.shape[0]
        out_a.append((row_q if q_is_a else row_s).cpu().numpy())
        out_b.append((row_s if q_is_a else row_q).cpu().numpy())
    return np.concatenate(out_a), np.concatenate(out_b)


def _larger_tables():
    a = rand_side(3201, 40_000, 24, 20_000_000, 900)
    b = uniform_side(3202, 600_000, 24, 20_000_000, 150)
    return (a.chrom, a.start, a.end), (b.chrom, b.start, b.end), 24


def _gloo_tables(skew):
    from test_distributed_gloo import _uniform_tables

    a, b = _uniform_tables(skew=skew)
    return a, b, 7


@gpu
@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("tables", ["plain", "skew", "larger"])
def test_ranks_on_one_gpu_equal_the_oracle_on_the_whole_tables(two_engines, tables, world):
    a, b, n_chrom = _larger_tables() if tables == "larger" else _gloo_tables(tables == "skew")
    ra, rb = ora.c_inner(ora.Side(*a), ora.Side(*b), "sweep")
    assert ra.shape[0] > 1000
    if tables == "skew" and world > 1:      # the dominant chromosome must really be spread over the ranks
        from giql_amd import distributed as D

        assert sum(bool((b[0][D.unit_rows(a[0], b[0], n_chrom, world, r)[1]] == 2).any()) for r in range(world)) > 1
    got_a, got_b = _ranks(two_engines, a, b, n_chrom, world)
    assert np.array_equal(P.pair_words(got_a, got_b), P.pair_words(ra, rb))
    got_a, got_b = _ranks(two_engines, b, a, n_chrom, world)        # the fixed-length table as A
    assert np.array_equal(P.pair_words(got_a, got_b), P.pair_words(rb, ra))


@gpu
@pytest.mark.parametrize("world", [2, 3])
def test_a_rank_whose_shard_has_free_lengths_on_both_sides_has_no_plan(two_engines, world):
    from giql_amd import distributed as D

    a, b, n_chrom = _gloo_tables(False)
    eb = b[2].copy()
    rows = np.nonzero(b[0] == 5)[0]
    eb[rows] += (np.arange(rows.shape[0]) % 9).astype(np.int32)      # chromosome 5: B rows of nine lengths
    b = (b[0], b[1], eb)
    owners = [r for r in range(world) if bool((b[0][D.unit_rows(a[0], b[0], n_chrom, world, r)[1]] == 5).any())]
    assert len(owners) == 1
    got_a, got_b = _ranks(two_engines, a, b, n_chrom, world, none_on=owners)
    # the other ranks' plans stand: every pair but that rank's (collectively, the callers exchange pairs instead)
    ra, rb = ora.c_inner(ora.Side(*a), ora.Side(*b), "sweep")
    lost = np.unique(a[0][D.unit_rows(a[0], b[0], n_chrom, world, owners[0])[0]])
    mine = ~np.isin(a[0][ra], lost)
    assert 0 < int(mine.sum()) < ra.shape[0]
    assert np.array_equal(P.pair_words(got_a, got_b), P.pair_words(ra[mine], rb[mine]))


@gpu
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_contiguous_shards_with_id_offsets_and_no_index_maps(two_engines, world):
    """The form bench.py runs: tables sorted by chromosome, a shard a contiguous row range of each, the export adding
    the range's first global row (rid_add_a / rid_add_b)."""
    from giql_amd import distributed as D

    a, b, n_chrom = _larger_tables()
    oa, ob = np.argsort(a[0], kind="stable"), np.argsort(b[0], kind="stable")
    a, b = tuple(x[oa] for x in a), tuple(x[ob] for x in b)
    local_plan, expand = D.hip_local_plan(two_engines[0]), D.hip_expand(two_engines[1])
    for first, second in ((a, b), (b, a)):
        blocks = []
        for chroms in np.array_split(np.arange(n_chrom), world):
            a0, a1 = np.searchsorted(first[0], chroms[0], "left"), np.searchsorted(first[0], chroms[-1], "right")
            b0, b1 = np.searchsorted(second[0], chroms[0], "left"), np.searchsorted(second[0], chroms[-1], "right")
            plan = local_plan(first[0][a0:a1], first[1][a0:a1], first[2][a0:a1], (0, 0), second[0][b0:b1],
                              second[1][b0:b1], second[2][b0:b1], (0, 0), n_chrom, rid_add_a=int(a0), rid_add_b=int(b0))
            assert plan is not None
            blocks.append(plan)
        got_a, got_b = _expand_blocks(expand, blocks)
        ra, rb = ora.c_inner(ora.Side(*first), ora.Side(*second), "sweep")
        assert np.array_equal(P.pair_words(got_a, got_b), P.pair_words(ra, rb))


@gpu
def test_hip_local_plan_of_an_empty_shard_and_hip_expand_of_no_pairs(two_engines):
    from giql_amd import distributed as D

    a, b, n_chrom = _gloo_tables(False)
    z = np.zeros(0, np.int32)
    local_plan, expand = D.hip_local_plan(two_engines[0]), D.hip_expand(two_engines[1])
    for plan in (local_plan(z, z, z, (0, 0), *b, (0, 0), n_chrom), local_plan(*a, (0, 0), z, z, z, (0, 0), n_chrom)):
        q_is_a, q_rid, lo, cnt, s_rid, n_pairs = plan
        assert q_is_a is True and n_pairs == 0
        assert all(x.dtype == torch.int32 and tuple(x.shape) == (0,) for x in (q_rid, lo, cnt, s_rid))
        row_q, row_s = expand(q_rid, lo, cnt, s_rid, 0)
        assert tuple(row_q.shape) == (0,) == tuple(row_s.shape)
    # tables that share no chromosome: a plan without pairs is the empty plan too
    plan = local_plan(a[0], a[1], a[2], (0, 0), b[0] + np.int32(7), b[1], b[2], (0, 0), 14)
    assert plan is not None and plan[5] == 0 and all(int(x.shape[0]) == 0 for x in plan[1:5])
