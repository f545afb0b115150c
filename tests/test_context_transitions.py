"""Every change of input and of call sequence on one long-lived HIP context, against the C oracle.

A ``giql_hip_ctx`` speculates: each call starts from what the previous call saw -- the INNER join form and its fixed
length, the fixed-length B of SEMI / ANTI / COUNT, the NEAREST plan and layout, sides that arrived sorted, whether the
fused count may run, the density (``last_span``) that picks the bucket width, the sticky switch to the four-pass sort --
and checks the guess at its own read-back (``giql_amd/csrc/giql_hip.hip``; the engine adds ``_pairs_guess``).  A guess
that is not checked properly shows only on the call AFTER a change of input, which hand-picked sequences rarely reach:
round 4's one state bug (ties of NEAREST / group_rows in input order after pile-ups and a dense table, commit 25a7a2b)
was found by a long random soak.  So here:

* Walk 1: per operator family, one fresh context walks an Eulerian circuit of the complete directed graph over the
  input classes (self-loops included): every ordered pair (X, Y) is a call on Y right after the context's last call
  on X.  Each visit runs the family twice; the second run must reach the path its class names (``SIGNATURES``).
  The ``row_pred`` family is SEMI / ANTI / COUNT over CONTAINS, WITHIN and DISTANCE and the within-distance join; the
  ``one_table`` family is CLUSTER, MERGE, MERGE with aggregates, MERGE with STRING_AGG and coverage (depth rows, then
  runs) over the class's B table, against the vectorised references of ``tests/_one_table_ref.py`` and
  ``tests/_coverage_ref.py``.
* Walk 2: one context, all seventeen operators, DISJOIN's three, CONTAINS' three and the two pair aggregates (over
  columns, over a per-pair expression) in a shuffled order per visit, with ``select`` / ``take_utf8`` / a plan of another
  operator / a pair aggregate / a call of the one-table family put between some plans and their fill -- which must then
  refuse (``GIQL_ERR_STATE``), as their columns of tests/test_plan_lifetime_gpu.py say: all of them begin a call.
* DISJOIN (self mode, reference mode, plan + fill through the raw ABI) walks the classes on which its path can
  differ, against the brute force of ``tests/_disjoin_ref.py``; its plan lives in the same workspace, and the
  context keeps one plan at a time (``ctx->kept``; ``tests/test_plan_lifetime_gpu.py`` has the rule cell by cell).
* CONTAINS / WITHIN (the join, the join with the sides exchanged, plan + fill through the raw ABI) walk the classes on
  which its path can differ, against the brute force of ``tests/_contain_ref.py``; its plan is the third kind the
  context can keep.
* Leg 3: the sticky four-pass fallback after a bucket too large for the bucket stage, reached from every class.
* Leg 4: production density on a default context: every ordered pair of bucket widths.

Pairs are compared as sorted multisets, per-row outputs exactly, NEAREST rows by the (start, end) of the matched row
(ties count), group_rows by its groups (``tools/soak_ops.py``).
"""

import functools

import numpy as np
import pytest

from oracle import pyoracle as ora

torch = pytest.importorskip("torch")


# ---------------------------------------------------------------- the schedule (pure; checked on the CPU below)
def eulerian_circuit(k: int) -> list:
    """Visit order over ``k`` classes that takes every ordered pair (i, j), i == j included, exactly once as two
    consecutive visits: an Eulerian circuit of the complete directed graph with self-loops (Hierholzer), from 0."""
    unused = {v: list(range(k - 1, -1, -1)) for v in range(k)}
    stack, circuit = [0], []
    while stack:
        v = stack[-1]
        if unused[v]:
            stack.append(unused[v].pop())
        else:
            circuit.append(stack.pop())
    return circuit[::-1]


@pytest.mark.parametrize("k", [1, 2, 5, 15, 16])
def test_schedule_takes_every_ordered_pair_once(k):
    walk = eulerian_circuit(k)
    assert len(walk) == k * k + 1 and walk[0] == walk[-1] == 0
    edges = list(zip(walk, walk[1:]))
    assert sorted(edges) == [(i, j) for i in range(k) for j in range(k)]


# ---------------------------------------------------------------- input classes
BS_FUSE_WCAP = 1 << 15     # longest query row the fused count's windows allow for (bucket_sort.hip.h)
BS_BIG_MAX = 1 << 18       # rows of one bucket the bucket stage sorts at all (bucket_sort.hip.h)


def _rows(r, n, nch, span, lens, lo=0):
    """n rows on nch chromosomes, starts uniform in [lo, lo + span), lengths ``lens`` (an int: fixed; a pair:
    uniform in [lens[0], lens[1]))."""
    ch = r.integers(0, nch, n).astype(np.int32)
    st = (lo + r.integers(0, span, n)).astype(np.int32)
    ln = np.full(n, lens, np.int64) if np.isscalar(lens) else r.integers(lens[0], lens[1], n)
    return ora.Side(ch, st, (st + ln).astype(np.int32))


def _density_span(n_b, per_65536):
    """The axis length over which n_b rows have per_65536 rows per 65,536 positions."""
    return int(n_b * 65536 / per_65536)


def _dense(seed, n_b, per_65536, n_a=2000, b_lens=150):
    """A B at a given density on one chromosome (fixed length 150 unless ``b_lens`` says otherwise), a short
    variable-length A over the same axis."""
    r = np.random.default_rng(seed)
    span = _density_span(n_b, per_65536)
    return _rows(r, n_a, 1, span, (1, 300)), _rows(r, n_b, 1, span, b_lens), 1


def _build_classes():
    out = {}
    r = np.random.default_rng(3001)
    out["general"] = (_rows(r, 3000, 4, 8_000_000, (1, 2000)), _rows(r, 20_000, 4, 8_000_000, (1, 800)), 4)
    out["uniform_b"] = (_rows(r, 3000, 4, 8_000_000, (1, 2000)), _rows(r, 20_000, 4, 8_000_000, 150), 4)
    out["uniform_a"] = (_rows(r, 20_000, 4, 8_000_000, 200), _rows(r, 3000, 4, 8_000_000, (1, 2000)), 4)
    out["larger_first"] = (_rows(r, 16_000, 4, 8_000_000, (1, 1500)), _rows(r, 4000, 4, 8_000_000, (1, 1500)), 4)
    a, b = _rows(r, 3000, 4, 8_000_000, (1, 2000)), _rows(r, 20_000, 4, 8_000_000, (1, 800))
    sa, sb = np.lexsort((a.start, a.chrom)), np.lexsort((b.start, b.chrom))
    out["presorted"] = (ora.Side(a.chrom[sa], a.start[sa], a.end[sa]), ora.Side(b.chrom[sb], b.start[sb], b.end[sb]), 4)
    # ~1 % of A inverted (raw end < start: irregular in every encoding), A 1-based closed beside a 0-based half-open B
    a = _rows(r, 3000, 3, 5_000_000, (1, 2000))
    inv = r.random(a.n) < 0.01
    a.end[inv] = a.start[inv] - 1 - r.integers(0, 5, int(inv.sum())).astype(np.int32)
    off = ora.ENCODING_OFFSETS[("1based", "closed")]
    out["irregular"] = (ora.Side(a.chrom, a.start, a.end, *off), _rows(r, 20_000, 3, 5_000_000, (1, 800)), 3)
    # runs of ~100 equal starts in B (NEAREST's two-sort plan)
    b = _rows(r, 20_000, 2, 4_000_000, (1, 3000))
    b.start[:] = (r.integers(0, 200, b.n) * 20_000).astype(np.int32)
    b.end[:] = b.start + r.integers(1, 3000, b.n).astype(np.int32)
    out["pileups"] = (_rows(r, 3000, 2, 4_000_000, (1, 2000)), b, 2)
    out["many_chroms"] = (_rows(r, 3000, 40, 2_000_000, (1, 2000)), _rows(r, 20_000, 40, 2_000_000, (1, 800)), 40)
    out["negative"] = (_rows(r, 3000, 3, 6_000_000, (1, 2000), lo=-3_000_000),
                       _rows(r, 20_000, 3, 6_000_000, (1, 800), lo=-3_000_000), 3)
    a, b, nch = _dense(3002, 100_000, 1000)
    a.end[:5] = a.start[:5] + np.arange(40_000, 65_000, 5000, dtype=np.int32)   # longer than BS_FUSE_WCAP
    out["long_rows"] = (a, b, nch)
    out["w16"] = _dense(3016, 100_000, 1000)
    # the narrow ones: lengths 100-199.  A fixed-length B is linearised on the aligned axis (2^24-position blocks),
    # whose span -- the density guess -- makes a table of a few 100k rows look sparse there: the narrow widths of
    # fixed-length tables are Leg 4's (production sizes).  And rows sharing a start differ in their end here: with a
    # fixed length, rows of equal start are equal rows, and an order among them that ignores the end cannot be told
    # from the right one (the 25a7a2b bug returned exactly such ties in input order)
    out["w15"] = _dense(3015, 100_000, 4000, b_lens=(100, 200))
    out["w14"] = _dense(3014, 150_000, 8000, b_lens=(100, 200))
    out["w13"] = _dense(3013, 250_000, 18_000, b_lens=(100, 200))
    out["sparse"] = _dense(3030, 20_000, 30)
    return out


def _oversized():
    """~300k B rows inside 4,000 positions of one chromosome -- more than BS_BIG_MAX rows in any bucket -- and a few
    rows of both sides spread over 10M positions, so that the table's own span asks for the bucket stage."""
    r = np.random.default_rng(3099)
    n_pile, n_wide = BS_BIG_MAX + 40_000, 50
    st = np.concatenate([r.integers(0, 4000, n_pile), r.integers(0, 10_000_000, n_wide)]).astype(np.int32)
    b = ora.Side(np.zeros(st.size, np.int32), st, st + 150)
    sa = np.concatenate([[100, 2500], r.integers(10_000, 10_000_000, 18)]).astype(np.int32)
    a = ora.Side(np.zeros(sa.size, np.int32), sa, sa + r.integers(1, 100, sa.size).astype(np.int32))
    return a, b, 1


SIGNATURES = {   # the settled (second) INNER call of a visit: it reached the path its class names
    "general": lambda st: st["join_form"] == "general",
    "uniform_b": lambda st: st["join_form"] == "uniform_b",
    "uniform_a": lambda st: st["join_form"] == "uniform_a",
    "larger_first": lambda st: st["swapped"],
    "presorted": lambda st: st["presorted"],
    "irregular": lambda st: st["n_irregular_a"] > 0,
    "pileups": lambda st: True,                     # (its path is NEAREST's two-sort plan: checked by its results)
    "many_chroms": lambda st: True,                 # (the index declines it: INDEX_DECLINES)
    "negative": lambda st: True,                    # (the index declines it: INDEX_DECLINES)
    "long_rows": lambda st: not st["count_fused"],      # (w16 with a few query rows too long for the fused count)
    "w16": lambda st: st["sort_local"] and st["bucket_bits"] == 16,
    # (INNER keys its sides on the 2^24-aligned axis, whose span makes these tables look sparse: its settled call takes
    # 16-bit buckets here.  The width each density asks for is asserted on the operators that sort on the tight span --
    # SEMI / ANTI / COUNT and NEAREST, SETTLED_WIDTH below -- and for INNER at production sizes, Leg 4)
    "w15": lambda st: st["sort_local"],
    "w14": lambda st: st["sort_local"],
    "w13": lambda st: st["sort_local"],
    "sparse": lambda st: not st["sort_local"],
}
INDEX_DECLINES = {"many_chroms": "chromosomes", "negative": "aligned axis"}   # class -> words of the documented reason
INDEX_QUERY_DECLINES = {"irregular", "long_rows"}   # query sides the indexed join may refuse (the ordinary join answers)
WIDTHS = {"w16": 16, "w15": 15, "w14": 14, "w13": 13}
WIDTH_FAMILIES = ("row", "nearest")   # sorts on the tight span: every settled call takes the width of its density
# (the ``row_pred`` family sorts on the tight span of its own call too -- each form reads its spans back and sets the
# density before it sorts -- but the statistics name the side sorted LAST, and COUNT over WITHIN sorts the small left
# table last (it is the inner side of the CONTAINS plan): its settled calls report A's form, not the width B's density
# asks for, so the family is not one of these)
# (the ``one_table`` family -- CLUSTER, MERGE and its aggregates, coverage -- is not one either: cluster_front and
# coverage's front sort before anything of their own call is read back, on ``guess.last_span`` as the previous call left
# it, and end in collect_spans and ``stats.span`` without note_span -- they read the density and never set it, as
# DISJOIN does.  A context that only ever ran this family keeps the fresh context's guess (a human-genome-sized axis),
# under which every class here is sparse: four passes on every call, asserted in Walk 1; the widths are met in Walk 2,
# after other operators' spans, and forced one by one in tests/test_one_table_paths.py)


@functools.lru_cache(maxsize=None)
def classes():
    return _build_classes()


NAMES = ["general", "uniform_b", "uniform_a", "larger_first", "presorted", "irregular", "pileups", "many_chroms",
         "negative", "long_rows", "w16", "w15", "w14", "w13", "sparse"]


def test_class_constructions_are_what_they_claim():
    """CPU: the classes have the shapes their names promise (densities, lengths, orders, chromosome counts)."""
    cl = classes()
    assert sorted(cl) == sorted(NAMES) and sorted(SIGNATURES) == sorted(NAMES)
    for name, w in WIDTHS.items():
        a, b, _ = cl[name]
        per = b.n * 65536 / (int(b.end.max()) - int(b.start.min()))
        lo, hi = (300, 2800) if w == 16 else (2800 * 2 ** (15 - w), 2800 * 2 ** (16 - w))
        assert lo < per <= hi, (name, per)
        assert (len(np.unique(b.end - b.start)) == 1) == (w == 16), name
        if w <= 15:     # rows of equal start with different ends
            s = np.lexsort((b.end, b.start))
            assert np.sum((np.diff(b.start[s]) == 0) & (np.diff(b.end[s]) != 0)) > 1000, name
        assert a.n * 65536 / (int(b.end.max()) - int(b.start.min())) < 300     # A alone stays in the four passes
    a, b, _ = cl["sparse"]
    assert b.n * 65536 / (int(b.end.max()) - int(b.start.min())) < 300
    assert (cl["long_rows"][0].end - cl["long_rows"][0].start).max() > BS_FUSE_WCAP
    assert cl["larger_first"][0].n == 4 * cl["larger_first"][1].n
    a, b, _ = cl["presorted"]
    for s in (a, b):
        assert np.all(np.diff(s.chrom.astype(np.int64) * 2**32 + s.start) >= 0)
    a = cl["irregular"][0]
    assert 0.005 < np.mean(a.ce <= a.cs) < 0.02 and np.all((a.end < a.start) == (a.ce <= a.cs))
    _, b, _ = cl["pileups"]
    assert np.unique(b.start, return_counts=True)[1].min() > 32
    assert cl["many_chroms"][2] == 40 and cl["negative"][0].start.min() < 0 and cl["negative"][1].start.min() < 0
    a, b, _ = _oversized()
    assert np.sum(b.start < 4000) > BS_BIG_MAX and b.start.max() > 9_000_000
    # the merged regions of the B tables at distance 0 (the ``one_table`` family): between them every band of region
    # lengths on which the aggregate kernels take another path -- one row, inside a wave, inside a 256-row tile, across
    # tiles inside one 64-tile fold step, across fold steps
    import _one_table_ref as V

    lengths = {name: V.Layout(cl[name][1].chrom, cl[name][1].start, cl[name][1].end, 0).count for name in NAMES}
    bands = {"1": (1, 1), "2-63": (2, 63), "64-255": (64, 255), "256-16383": (256, 16_383), "16384-": (16_384, 2**31)}
    met = {band: [name for name in NAMES if np.any((lengths[name] >= lo) & (lengths[name] <= hi))] for band, (lo, hi) in bands.items()}
    assert all(met.values()), met
    assert lengths["general"].max() <= 63 and "general" in met["1"] and "general" in met["2-63"]
    assert "w16" in met["64-255"] and "w15" in met["256-16383"] and "w15" in met["16384-"]
    assert all(lengths[name].max() >= 16_384 for name in ("w14", "w13"))
    assert all(lengths[name].sum() == cl[name][1].n for name in NAMES)


# ---------------------------------------------------------------- GPU side: resident sides, cached oracle answers
def _dev(side):
    from giql_amd.engine import DeviceSide

    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.int32)).to("cuda:0")
    return DeviceSide(t(side.chrom), t(side.start), t(side.end), side.start_off, side.end_off)


@functools.lru_cache(maxsize=None)
def resident(name):
    a, b, nch = _oversized() if name == "oversized" else classes()[name]
    return a, b, nch, _dev(a), _dev(b)


@functools.lru_cache(maxsize=None)
def want(name, what, *args):
    a, b, _nch, _da, _db = resident(name)
    if what == "pairs":
        return ora.sort_pairs(*ora.c_inner(a, b, "sweep"))
    if what == "semi":
        return ora.c_semi_anti(a, b, False)
    if what == "anti":
        return ora.c_semi_anti(a, b, True)
    if what == "count":
        return ora.c_count(a, b, "sweep")
    if what == "nearest":
        return ora.c_nearest_k1(a, b, signed=args[0], method="sweep")
    if what == "nearest_k":
        return ora.c_nearest_k(a, b, args[0])
    raise AssertionError(what)


def _rows_equal(b, got, exp):
    ok = exp >= 0
    return (np.array_equal(got >= 0, ok) and np.array_equal(b.start[got[ok]], b.start[exp[ok]])
            and np.array_equal(b.end[got[ok]], b.end[exp[ok]]))


def _pairs(ra, rb):
    return ora.sort_pairs(ra.cpu().numpy(), rb.cpu().numpy())


def _density_engine(monkeypatch):
    """A context with the production density rules but without the 2^21-row floor (giql_hip.hip reads the three
    variables in this order: the floor first, then the two density bounds it reset)."""
    from giql_amd.engine import HipEngine

    monkeypatch.setenv("GIQL_HIP_LOCAL_MIN_ROWS", "1")
    monkeypatch.setenv("GIQL_HIP_LOCAL_MIN_BUCKET_ROWS", "300")
    monkeypatch.setenv("GIQL_HIP_LOCAL_MAX_BUCKET_ROWS", "2800")
    e = HipEngine(0)
    monkeypatch.delenv("GIQL_HIP_LOCAL_MIN_ROWS")
    monkeypatch.delenv("GIQL_HIP_LOCAL_MIN_BUCKET_ROWS")
    monkeypatch.delenv("GIQL_HIP_LOCAL_MAX_BUCKET_ROWS")
    return e


class Log:
    """Every call of a walk: (family, class, round, operator, stats of that call)."""

    def __init__(self):
        self.calls = []

    def add(self, eng, family, name, rnd, op):
        self.calls.append((family, name, rnd, op, eng.stats()))

    def transitions(self, family):
        seq = [c[1] for c in self.calls if c[0] == family]
        return set(zip(seq, seq[1:]))


# ---- the operators: each runs one call sequence on (class) and checks it against the oracle
def op_inner_join(eng, name, log, fam, rnd):
    _a, _b, nch, da, db = resident(name)
    ra, rb = eng.inner_join(da, db, nch)
    log.add(eng, fam, name, rnd, "inner_join")
    assert np.array_equal(_pairs(ra, rb), want(name, "pairs")), (name, "inner_join")


def _into(eng, name, cap):
    _a, _b, nch, da, db = resident(name)
    ra = torch.full((cap,), -7, dtype=torch.int32, device="cuda:0")
    rb = torch.full((cap,), -7, dtype=torch.int32, device="cuda:0")
    return ra, rb, eng.inner_join_into(da, db, nch, ra, rb)


def op_into_exact(eng, name, log, fam, rnd):
    w = want(name, "pairs")
    ra, rb, n = _into(eng, name, w.shape[0])
    log.add(eng, fam, name, rnd, "into_exact")
    assert n == w.shape[0] and np.array_equal(_pairs(ra, rb), w), (name, "into_exact")


def op_into_short(eng, name, log, fam, rnd):
    from giql_amd import _lib

    w = want(name, "pairs")
    n = w.shape[0]
    assert n > 0
    with pytest.raises(_lib.GiqlHipError) as exc:
        _into(eng, name, n - 1)
    log.add(eng, fam, name, rnd, "into_short")
    assert exc.value.code == _lib.GIQL_ERR_CAPACITY and eng.last_pairs == n, (name, str(exc.value), eng.last_pairs, n)
    ra = torch.empty(n, dtype=torch.int32, device="cuda:0")
    rb = torch.empty(n, dtype=torch.int32, device="cuda:0")
    eng.inner_fill(ra, rb)
    assert np.array_equal(_pairs(ra, rb), w), (name, "fill after GIQL_ERR_CAPACITY")


def op_into_ample(eng, name, log, fam, rnd):
    w = want(name, "pairs")
    ra, rb, n = _into(eng, name, w.shape[0] + 4096)
    log.add(eng, fam, name, rnd, "into_ample")
    assert n == w.shape[0] and np.array_equal(_pairs(ra[:n], rb[:n]), w), (name, "into_ample")
    if rnd == 2:    # (a call whose guesses missed may leave its abandoned attempt's pairs past the count: giql_hip.h)
        assert int((ra[n:] != -7).sum()) == 0 and int((rb[n:] != -7).sum()) == 0, (name, "written past the count")


def op_plan_fill(eng, name, log, fam, rnd, intruder=None):
    from giql_amd import _lib

    _a, _b, nch, da, db = resident(name)
    w = want(name, "pairs")
    n = eng.inner_plan(da, db, nch)
    log.add(eng, fam, name, rnd, "plan")
    assert n == w.shape[0], (name, "plan count")
    ra = torch.empty(n, dtype=torch.int32, device="cuda:0")
    rb = torch.empty(n, dtype=torch.int32, device="cuda:0")
    if intruder is not None:
        # a call that reuses the plan's workspace between the plan and its fill: the plan is gone
        intruder(eng, name)
        for consume in (lambda: eng.inner_fill(ra, rb), lambda: eng.plan_export(ra, ra, ra, rb)):
            with pytest.raises(_lib.GiqlHipError) as exc:
                consume()
            assert exc.value.code == _lib.GIQL_ERR_STATE and "without a successful inner_plan" in str(exc.value), exc.value
        assert eng.inner_plan(da, db, nch) == n
    eng.inner_fill(ra, rb)
    assert np.array_equal(_pairs(ra, rb), w), (name, "plan + fill")


def op_semi(eng, name, log, fam, rnd):
    _a, _b, nch, da, db = resident(name)
    got = eng.semi_join(da, db, nch).cpu().numpy()
    log.add(eng, fam, name, rnd, "semi")
    assert np.array_equal(got, want(name, "semi")), (name, "semi")


def op_anti(eng, name, log, fam, rnd):
    _a, _b, nch, da, db = resident(name)
    got = eng.anti_join(da, db, nch).cpu().numpy()
    log.add(eng, fam, name, rnd, "anti")
    assert np.array_equal(got, want(name, "anti")), (name, "anti")


def op_count(eng, name, log, fam, rnd):
    _a, _b, nch, da, db = resident(name)
    got = eng.count_overlaps(da, db, nch).cpu().numpy()
    log.add(eng, fam, name, rnd, "count")
    assert np.array_equal(got, want(name, "count")), (name, "count")


def _nearest_refused(eng, call):
    """Inverted rows: NEAREST refuses them (the walk goes on on the same context: it must stay usable)."""
    from giql_amd import _lib

    with pytest.raises(_lib.GiqlHipError) as exc:
        call()
    assert exc.value.code == _lib.GIQL_ERR_INVALID, exc.value


def op_nearest(eng, name, log, fam, rnd):
    _a, b, nch, da, db = resident(name)
    signed = len(log.calls) % 2 == 1                # alternating signed / unsigned along the walk
    if name == "irregular":
        _nearest_refused(eng, lambda: eng.nearest(da, db, nch, signed=signed))
        log.add(eng, fam, name, rnd, "nearest")
        return
    idx, dist = eng.nearest(da, db, nch, signed=signed)
    log.add(eng, fam, name, rnd, "nearest")
    wi, wd = want(name, "nearest", signed)
    assert np.array_equal(dist.cpu().numpy(), wd), (name, "nearest distance", signed)
    assert _rows_equal(b, idx.cpu().numpy(), wi), (name, "nearest rows", signed)


def op_nearest_k(eng, name, log, fam, rnd):
    _a, b, nch, da, db = resident(name)
    if name == "irregular":
        _nearest_refused(eng, lambda: eng.nearest_k(da, db, nch, 3))
        log.add(eng, fam, name, rnd, "nearest_k")
        return
    idx, dist = eng.nearest_k(da, db, nch, 3)
    log.add(eng, fam, name, rnd, "nearest_k")
    wi, wd = want(name, "nearest_k", 3)
    assert np.array_equal(dist.cpu().numpy(), wd), (name, "nearest_k distance")
    assert _rows_equal(b, idx.cpu().numpy(), wi), (name, "nearest_k rows")


def op_group_rows(eng, name, log, fam, rnd):
    _a, b, nch, _da, db = resident(name)
    gid, rep = eng.group_rows(db, nch)
    log.add(eng, fam, name, rnd, "group_rows")
    gid, rep = gid.cpu().numpy(), rep.cpu().numpy()
    trip = np.stack([b.chrom, b.start, b.end], 1)
    assert rep.shape[0] == np.unique(trip, axis=0).shape[0], (name, "group count")
    assert np.array_equal(trip[rep[gid]], trip), (name, "group rows")


def op_index(eng, name, log, fam, rnd):
    from giql_amd import _lib

    _a, _b, nch, da, db = resident(name)
    try:
        index = eng.index_create(db, nch)
    except _lib.GiqlHipError as exc:
        log.add(eng, fam, name, rnd, "index_declined")
        assert exc.code == _lib.GIQL_ERR_STATE and name in INDEX_DECLINES, (name, str(exc))
        assert INDEX_DECLINES[name] in str(exc), (name, str(exc))
        return
    assert name not in INDEX_DECLINES, (name, "an index was built")
    try:
        ra, rb = eng.inner_join_indexed(da, index)
        log.add(eng, fam, name, rnd, "indexed")
        assert np.array_equal(_pairs(ra, rb), want(name, "pairs")), (name, "indexed")
    except _lib.GiqlHipError as exc:
        log.add(eng, fam, name, rnd, "indexed_declined")
        assert exc.code == _lib.GIQL_ERR_STATE and name in INDEX_QUERY_DECLINES, (name, str(exc))
    finally:
        index.close()


# ---- DISJOIN: target = the class's A, reference = its B (self mode: A alone); truth = tests/_disjoin_ref.py's
# vectorised brute force, anchored row by row in tests/test_disjoin.py
DISJOIN_NAMES = ["general", "presorted", "irregular", "pileups", "many_chroms", "negative", "w16", "w13", "sparse"]


@functools.lru_cache(maxsize=None)
def want_disjoin(name, mode):
    from _disjoin_ref import brute_force_arrays

    a, b, _nch, _da, _db = resident(name)
    i64 = lambda s: [s.chrom.astype(np.int64), s.cs.astype(np.int64), s.ce.astype(np.int64)]
    out = brute_force_arrays(*i64(a)) if mode == "self" else brute_force_arrays(*i64(a), *i64(b))
    out[:, 1] -= a.start_off
    out[:, 2] -= a.end_off
    return out


def _pieces(parent, ds, de):
    return np.stack([parent.cpu().numpy(), ds.cpu().numpy(), de.cpu().numpy()], 1).astype(np.int64)


def _disjoin_call(eng, name, log, fam, rnd, mode):
    _a, _b, nch, da, db = resident(name)
    reference = None if mode == "self" else db
    if name == "irregular":      # inverted rows in A: the error names the side that holds them
        with pytest.raises(ValueError, match="the target has a row with start > end"):
            eng.disjoin(da, reference, nch)
        log.add(eng, fam, name, rnd, "disjoin_" + mode)
        return
    got = _pieces(*eng.disjoin(da, reference, nch))
    log.add(eng, fam, name, rnd, "disjoin_" + mode)
    w = want_disjoin(name, mode)
    assert got.shape == w.shape and np.array_equal(got, w), (name, "disjoin", mode)


def op_disjoin_self(eng, name, log, fam, rnd):
    _disjoin_call(eng, name, log, fam, rnd, "self")


def op_disjoin_ref(eng, name, log, fam, rnd):
    _disjoin_call(eng, name, log, fam, rnd, "reference")


def op_disjoin_plan_fill(eng, name, log, fam, rnd, intruder=None):
    from _disjoin_ref import fill_raw, plan_raw
    from giql_amd import _lib

    _a, _b, nch, da, db = resident(name)
    rc, n = plan_raw(eng, da, db, nch)
    log.add(eng, fam, name, rnd, "disjoin_plan")
    outs = [torch.full((max(n, 8),), -7, dtype=torch.int32, device="cuda:0") for _ in range(3)]
    if name == "irregular":
        assert rc == _lib.GIQL_ERR_INVALID and b"the target has a row" in eng._L.giql_hip_last_error(), (name, rc)
        assert fill_raw(eng, outs, 8) == _lib.GIQL_ERR_STATE and all(int((o != -7).sum()) == 0 for o in outs)
        return
    w = want_disjoin(name, "reference")
    assert (rc, n) == (0, w.shape[0]), (name, "disjoin plan", rc, n)
    if intruder is not None:
        intruder(eng, name)          # reuses the workspace the plan lives in: the plan is gone
        assert fill_raw(eng, outs, n) == _lib.GIQL_ERR_STATE, (name, intruder.__name__)
        assert b"without a successful disjoin_plan" in eng._L.giql_hip_last_error()
        assert all(int((o != -7).sum()) == 0 for o in outs), (name, "a refused fill wrote")
        assert plan_raw(eng, da, db, nch) == (0, n)
    assert fill_raw(eng, outs, n) == 0
    got = _pieces(*(o[:n] for o in outs))
    assert np.array_equal(got, w), (name, "disjoin plan + fill")


DISJOIN_OPS = [op_disjoin_self, op_disjoin_ref, op_disjoin_plan_fill]


# ---- CONTAINS / WITHIN: outer = the class's A, inner = its B (WITHIN: the sides exchanged); truth = the brute force
# of tests/_contain_ref.py, or its sort-based reference (anchored on the brute force in tests/test_contain.py) where
# the brute force would take more than a few seconds
CONTAIN_NAMES = ["general", "uniform_b", "irregular", "pileups", "many_chroms", "negative", "w15", "sparse"]
CONTAIN_UNIFORM = {"contains": {"uniform_b", "long_rows", "w16", "sparse"}, "within": {"uniform_a"}}   # word -> classes whose inner side has one length
CONTAIN_MAX_CELLS = 10**8


@functools.lru_cache(maxsize=None)
def want_contain(name, word):
    import _contain_ref as C

    a, b, _nch, _da, _db = resident(name)
    i64 = lambda s: (s.chrom.astype(np.int64), s.cs.astype(np.int64), s.ce.astype(np.int64))
    outer, inner = (i64(a), i64(b)) if word == "contains" else (i64(b), i64(a))
    return C.truth(outer, inner, max_cells=CONTAIN_MAX_CELLS)


def _contain_call(eng, name, log, fam, rnd, word):
    _a, _b, nch, da, db = resident(name)
    outer, inner = (da, db) if word == "contains" else (db, da)
    ro, ri = eng.contain_join(outer, inner, nch)
    log.add(eng, fam, name, rnd, word)
    st = log.calls[-1][4]
    w = want_contain(name, word)
    assert st["n_out"] == w.shape[0] and np.array_equal(_pairs(ro, ri), w), (name, word)
    # (the form is read back in every plan, never guessed: it holds on a first call after another class too)
    assert st["join_form"] == ("uniform_b" if name in CONTAIN_UNIFORM[word] else "general"), (name, word, st["join_form"])


def op_contain_join(eng, name, log, fam, rnd):
    _contain_call(eng, name, log, fam, rnd, "contains")


def op_contain_within(eng, name, log, fam, rnd):
    _contain_call(eng, name, log, fam, rnd, "within")


def _contain_plan_raw(eng, outer, inner, nch):
    import ctypes

    co, ci = outer.c_struct(), inner.c_struct()
    n = ctypes.c_int64(-1)
    rc = eng._L.giql_hip_contain_plan_dev(eng._h, ctypes.byref(co), ctypes.byref(ci), nch, eng._stream(), ctypes.byref(n))
    return rc, n.value


def op_contain_plan_fill(eng, name, log, fam, rnd, intruder=None):
    from giql_amd import _lib

    _a, _b, nch, da, db = resident(name)
    w = want_contain(name, "contains")
    rc, n = _contain_plan_raw(eng, da, db, nch)
    log.add(eng, fam, name, rnd, "contain_plan")
    assert (rc, n) == (0, w.shape[0]), (name, "contain plan", rc, n)
    ro = torch.full((max(n, 8),), -7, dtype=torch.int32, device="cuda:0")
    ri = torch.full((max(n, 8),), -7, dtype=torch.int32, device="cuda:0")
    fill = lambda: eng._L.giql_hip_contain_fill_dev(eng._h, ro.data_ptr(), ri.data_ptr(), n, eng._stream())
    if intruder is not None:
        intruder(eng, name)          # reuses the workspace the plan lives in: the plan is gone
        assert fill() == _lib.GIQL_ERR_STATE, (name, intruder.__name__)
        assert b"without a successful contain_plan" in eng._L.giql_hip_last_error()
        assert int((ro != -7).sum()) == 0 and int((ri != -7).sum()) == 0, (name, "a refused fill wrote")
        assert _contain_plan_raw(eng, da, db, nch) == (0, n)
    assert fill() == 0
    assert np.array_equal(_pairs(ro[:n], ri[:n]), w), (name, "contain plan + fill")


CONTAIN_OPS = [op_contain_join, op_contain_within, op_contain_plan_fill]


# ---- SEMI / ANTI / COUNT over CONTAINS, WITHIN and DISTANCE, and the within-distance join: they read and write the
# density the next call's sort follows (``guess.last_span``) like the INTERSECTS forms.  One predicate per visit, in
# turn: its first round runs on what the previous visit's predicate and class left, its second on its own (the walk's
# time is the brute-force references', many times the ``row`` family's: one predicate a visit, not all three).
# Truth = the pair references of the contain family reduced per left row (tests/_rows_ref.py) and the chunked brute
# force of the window predicate.
ROW_PREDS = (("contains", None), ("within", None), ("within_distance", 1000))
ROW_PRED_CALLS = 2 * 4      # log entries of one visit: two rounds of SEMI, ANTI, COUNT, the join


def _round_pred(log, fam):
    return ROW_PREDS[(sum(c[0] == fam for c in log.calls) // ROW_PRED_CALLS) % len(ROW_PREDS)]


@functools.lru_cache(maxsize=None)
def want_row_pred(name, predicate, n):
    """(semi ids, anti ids, counts) per row of the class's A."""
    import _rows_ref as R

    a, b, _nch, _da, _db = resident(name)
    if predicate == "contains":
        return R.reduce_pairs(want_contain(name, "contains"), a.n)
    if predicate == "within":
        return R.reduce_pairs(R.transpose(want_contain(name, "within")), a.n)
    counts = R.window_counts(a.chrom, a.cs, a.ce, b.chrom, b.cs, b.ce, n)
    ids = np.arange(a.n, dtype=np.int64)
    return ids[counts > 0], ids[counts == 0], counts


def _distance_refused(eng, name, predicate, call):
    """DISTANCE refuses the class with inverted rows, naming the side (the walk goes on on the same context)."""
    from giql_amd.engine import InvertedRows

    if not (predicate == "within_distance" and name == "irregular"):
        return False
    with pytest.raises(InvertedRows) as exc:
        call()
    assert exc.value.sides == ("a",), (name, exc.value.sides)
    return True


def op_semi_pred(eng, name, log, fam, rnd):
    _a, _b, nch, da, db = resident(name)
    predicate, n = _round_pred(log, fam)
    for anti in (False, True):
        what = "anti_pred" if anti else "semi_pred"
        if _distance_refused(eng, name, predicate, lambda: eng.semi_anti_pred(da, db, nch, predicate, anti, n)):
            log.add(eng, fam, name, rnd, what)
            continue
        got = eng.semi_anti_pred(da, db, nch, predicate, anti, n).cpu().numpy()
        log.add(eng, fam, name, rnd, what)
        assert np.array_equal(got, want_row_pred(name, predicate, n)[1 if anti else 0]), (name, what, predicate)


def op_count_pred(eng, name, log, fam, rnd):
    _a, _b, nch, da, db = resident(name)
    predicate, n = _round_pred(log, fam)
    if _distance_refused(eng, name, predicate, lambda: eng.count_pred(da, db, nch, predicate, n)):
        log.add(eng, fam, name, rnd, "count_pred")
        return
    got = eng.count_pred(da, db, nch, predicate, n).cpu().numpy()
    log.add(eng, fam, name, rnd, "count_pred")
    assert np.array_equal(got, want_row_pred(name, predicate, n)[2]), (name, "count_pred", predicate)


def op_window_join(eng, name, log, fam, rnd):
    """The within-distance join (N = 1000 whatever the round's predicate: the plan is DISTANCE's own).  Its pairs are
    the reference's exactly when each is one of them, none comes twice and every left row has its count of them."""
    a, b, nch, da, db = resident(name)
    n = 1000
    if _distance_refused(eng, name, "within_distance", lambda: eng.window_join(da, db, nch, n)):
        log.add(eng, fam, name, rnd, "window_join")
        return
    ra, rb = (t.cpu().numpy().astype(np.int64) for t in eng.window_join(da, db, nch, n))
    log.add(eng, fam, name, rnd, "window_join")
    counts = want_row_pred(name, "within_distance", n)[2]
    assert np.array_equal(np.bincount(ra, minlength=a.n), counts), (name, "window_join counts")
    assert np.unique(ra * b.n + rb).size == ra.size, (name, "window_join: a pair twice")
    assert np.all((a.chrom[ra] == b.chrom[rb]) & (a.cs[ra] - n < b.ce[rb]) & (a.ce[ra] + n > b.cs[rb])), (name, "window_join")


# ---- CLUSTER, MERGE, MERGE with aggregates and with STRING_AGG over the class's B (raw coordinates: its offsets are 0),
# distance 0; truth = the vectorised reference of tests/_one_table_ref.py (held to the row-by-row ones in
# tests/test_one_table_ref.py), once per class and kept on the device.  All four go through cluster_front: they sort by
# start on the density another call left (``guess.last_span``), and leave it as they found it.
ONE_TABLE_AGGS = (("SUM", "f"), ("MAX", "f"), ("SUM", "i"), ("MIN", "i"))


@functools.lru_cache(maxsize=None)
def one_table(name):
    """``(layout, device inputs, device answers)`` of the class's B table."""
    import _one_table_ref as V

    _a, b, _nch, _da, _db = resident(name)
    r = np.random.default_rng(7000 + NAMES.index(name) if name in NAMES else 7099)
    lay = V.Layout(b.chrom, b.start, b.end, 0)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")
    cols = {"f": ((r.normal(0, 1000, b.n) * r.choice([1e-3, 1.0, 1e3], b.n)), r.random(b.n) >= 0.3),
            "i": (r.integers(-1_000_000, 1_000_000, b.n), r.random(b.n) >= 0.3)}
    letters, null = r.integers(97, 123, (b.n, 3), dtype=np.uint8), r.random(b.n) < 0.2
    words = [None if null[i] else b"%d:" % i + bytes(letters[i, :i % 4]) for i in range(b.n)]      # every value names its row
    lens = np.array([0 if w is None else len(w) for w in words], np.int64)
    inputs = {k: (dev(v), dev(ok.astype(np.uint8))) for k, (v, ok) in cols.items()}
    inputs["words"] = (dev(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)),
                       dev(np.frombuffer(b"".join(w or b"" for w in words), np.uint8).copy()), dev((~null).astype(np.uint8)))
    answers = {"ids": dev(lay.cluster_ids()),
               "rows": [dev(x.astype(np.int64 if k == 3 else np.int32)) for k, x in enumerate(lay.merge_rows())]}
    for func, c in ONE_TABLE_AGGS:
        vals, ok = lay.aggregate(func, *cols[c])
        answers[func, c] = (dev(vals), dev(ok))
    # a float SUM over k non-NULL values: within k * 2^-52 * sum|x_i| of fsum (tests/test_merge_aggregates_gpu.py)
    answers["bound"] = dev(lay.non_null(cols["f"][1]) * 2.0**-52 * lay.abs_sum(*cols["f"]))
    off, data, ok = lay.string_agg(words, b",")
    answers["str"] = (dev(off.astype(np.int32)), dev(np.frombuffer(data, np.uint8).copy()), dev(ok))
    return lay, inputs, answers


@functools.lru_cache(maxsize=None)
def _inverted_raw():
    """``irregular``'s A with its offsets set to 0, as CLUSTER / MERGE take a table: its inverted rows stay."""
    a = classes()["irregular"][0]
    assert np.any(a.end < a.start)
    return _dev(ora.Side(a.chrom, a.start, a.end))


def _merge_rows_equal(out, answers, what):
    assert all(g.shape == w.shape and torch.equal(g, w) for g, w in zip(out[:4], answers["rows"])), what


def op_cluster(eng, name, log, fam, rnd):
    from giql_amd import _lib

    _a, _b, nch, _da, db = resident(name)
    if name == "irregular":      # inverted rows are refused, and the very next call on the context is right
        with pytest.raises(_lib.GiqlHipError, match="need start <= end") as exc:
            eng.cluster(_inverted_raw(), nch, 0)
        assert exc.value.code == _lib.GIQL_ERR_INVALID, exc.value
    ids = eng.cluster(db, nch, 0)
    log.add(eng, fam, name, rnd, "cluster")
    assert torch.equal(ids, one_table(name)[2]["ids"]), (name, "cluster")


def op_merge(eng, name, log, fam, rnd):
    _a, _b, nch, _da, db = resident(name)
    out = eng.merge(db, nch, 0)
    log.add(eng, fam, name, rnd, "merge")
    _merge_rows_equal(out, one_table(name)[2], (name, "merge"))


def op_merge_agg(eng, name, log, fam, rnd):
    _a, _b, nch, _da, db = resident(name)
    _lay, inputs, answers = one_table(name)
    out = eng.merge_agg(db, nch, 0, [(f,) + inputs[c] for f, c in ONE_TABLE_AGGS])
    log.add(eng, fam, name, rnd, "merge_agg")
    _merge_rows_equal(out, answers, (name, "merge_agg"))
    for (func, c), (vals, ok) in zip(ONE_TABLE_AGGS, out[4:]):
        want, want_ok = answers[func, c]
        assert torch.equal(ok, want_ok) and vals.dtype == want.dtype, (name, func, c, "validity")
        if (func, c) == ("SUM", "f"):
            assert bool(((vals - want).abs() <= answers["bound"]).all()), (name, "SUM(f)")
        else:
            assert torch.equal(vals, want), (name, func, c)


def op_merge_str(eng, name, log, fam, rnd):
    _a, _b, nch, _da, db = resident(name)
    _lay, inputs, answers = one_table(name)
    out = eng.merge_agg(db, nch, 0, [("STRING_AGG",) + inputs["words"] + (b",",)])
    log.add(eng, fam, name, rnd, "merge_str")       # (the string fill is the last call: these stats name no sort)
    _merge_rows_equal(out, answers, (name, "merge_str"))
    assert all(g.shape == w.shape and torch.equal(g, w) for g, w in zip(out[4], answers["str"])), (name, "merge_str")


# ---- coverage over the class's B (raw coordinates, like the rest of the family): DISJOIN's front -- spans, 2n events,
# ONE sort by start, two flag scans -- in the workspace every other call carves, then its own breakpoint rows.  Like
# DISJOIN and the four operators above it sorts on the density another call left (``guess.last_span``) and leaves it as
# it found it: giql_hip_coverage_dev_impl ends in collect_spans and ``stats.span`` without note_span, and DESIGN.md says
# so.  Truth = the vectorised sweep of tests/_coverage_ref.py (held to the row-by-row one and to the sqlite-minted
# golden in tests/test_coverage.py), once per class and form, kept on the device.
@functools.lru_cache(maxsize=None)
def want_coverage(name, runs):
    from _coverage_ref import sweep_arrays

    _a, b, _nch, _da, _db = resident(name)
    rows = sweep_arrays(b.chrom, b.start, b.end, runs=runs)
    assert 0 < rows.shape[0] < 2 * b.n
    return [torch.from_numpy(np.ascontiguousarray(rows[:, k]).astype(np.int64 if k == 3 else np.int32)).to("cuda:0")
            for k in range(4)]


def op_coverage(eng, name, log, fam, rnd):
    """Depth rows in round 1, runs in round 2.  On ``irregular`` a table with inverted rows is refused first, naming the
    table; the call that follows on the same context must be right."""
    _a, _b, nch, _da, db = resident(name)
    runs = rnd == 2
    if name == "irregular":
        with pytest.raises(ValueError, match="the target has a row with start > end"):
            eng.coverage(_inverted_raw(), nch, runs=runs)
    out = eng.coverage(db, nch, runs=runs)
    log.add(eng, fam, name, rnd, "coverage")
    want = want_coverage(name, runs)
    assert all(g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w) for g, w in zip(out, want)), (name, "coverage", runs)
    assert log.calls[-1][4]["n_out"] == want[0].shape[0], (name, "coverage rows")


ONE_TABLE_OPS = [op_cluster, op_merge, op_merge_agg, op_merge_str, op_coverage]


# ---- the aggregates over a join's pairs per left row, over columns and over a per-pair expression.  They take ids, not
# tables: pair_agg_impl reads and writes no guess (its sorts are run_sort with as many passes as the ids have digits,
# whatever the context's sort switches and density say), so they have no Walk 1 of their own -- what they share with the
# rest is the workspace (claim_arena), the scans' status words and the plan the context keeps.  Their pairs are the
# class's own INNER join, sorted, at most PAIR_AGG_MAX_PAIRS of them from the front (every left row of the prefix but
# the last keeps all its pairs), handed over in a shuffled order; truth = tests/_pair_agg_ref.py and
# tests/_pair_expr_agg_ref.py on the same prefix, with the float SUM bound of tests/_stream_harness.py.
PAIR_AGG_MAX_PAIRS = 50_000
PAIR_AGGS = (("SUM", "vf"), ("AVG", "vf"), ("MIN", "vf"), ("MAX", "vf"), ("COUNT", "vf"), ("SUM", "vi"), ("MAX", "vi"))
PAIR_EXPR_FUNCS = ("SUM", "MIN", "COUNT")      # of ``a.ca + b.vi * 3``; beside them SUM(b.vf)


@functools.lru_cache(maxsize=None)
def pair_agg_case(name):
    """``(device inputs, host inputs)`` of the class: the pair prefix and the columns the aggregates read."""
    a, b, _nch, _da, _db = resident(name)
    r = np.random.default_rng(7500 + NAMES.index(name))
    pairs = want(name, "pairs")[:PAIR_AGG_MAX_PAIRS]
    pairs = pairs[r.permutation(pairs.shape[0])]
    host = {"ra": pairs[:, 0].astype(np.int32), "rb": pairs[:, 1].astype(np.int32),
            "vf": r.normal(0, 1000, b.n) * r.choice([1e-3, 1.0, 1e3], b.n), "vf.valid": (r.random(b.n) >= 0.3).astype(np.uint8),
            "vi": r.integers(-1_000_000, 1_000_000, b.n).astype(np.int64),
            "ca": r.integers(-1000, 1000, a.n).astype(np.int64), "ca.valid": (r.random(a.n) >= 0.3).astype(np.uint8)}
    assert host["ra"].shape[0] > 0
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0") for k, v in host.items()}, host


@functools.lru_cache(maxsize=None)
def want_pair_agg(name, expr):
    import _pair_agg_ref as R
    import _pair_expr_agg_ref as X
    import _stream_harness as H

    a = resident(name)[0]
    _dev_in, host = pair_agg_case(name)
    vf, vi = H._py_column(host, "vf"), H._py_column(host, "vi")
    if not expr:
        cols = {"vf": vf, "vi": vi}
        pairs, results = R.pair_aggregate(host["ra"], host["rb"], a.n, cols, list(PAIR_AGGS))
        mem = R.members(host["ra"], host["rb"], a.n)
        leaves = [H._pagg_leaf(f, w, [[cols[c][j] for j in m] for m in mem], c == "vf") for (f, c), w in zip(PAIR_AGGS, results)]
    else:
        tree, plain = _pair_tree(host), ("col", vf)
        aggs = [(f, tree) for f in PAIR_EXPR_FUNCS] + [("SUM", plain)]
        pairs, results, inputs = X.pair_expr_aggregate(host["ra"], host["rb"], a.n, aggs)
        leaves = [H._pagg_leaf(f, w, xs, src is plain) for (f, src), w, xs in zip(aggs, results, inputs)]
    return (np.array(pairs, np.int64),) + tuple(leaves)


def _pair_tree(cols):
    return ("+", ("a", cols["ca"], cols["ca.valid"]), ("*", ("b", cols["vi"]), ("lit", 3)))


def _pair_agg_call(eng, name, log, fam, rnd, expr):
    import _stream_harness as H

    a, b, _nch, _da, _db = resident(name)
    d, _host = pair_agg_case(name)
    if expr:
        aggs = [(f, ("expr", _pair_tree(d))) for f in PAIR_EXPR_FUNCS] + [("SUM", d["vf"], d["vf.valid"])]
    else:
        aggs = [(f, d[c], d["vf.valid"] if c == "vf" else None) for f, c in PAIR_AGGS]
    pairs, results = eng.pair_aggregate(d["ra"], d["rb"], a.n, b.n, aggs)
    what = "pair_expr_agg" if expr else "pair_agg"
    log.add(eng, fam, name, rnd, what)
    got = (pairs.cpu().numpy(),) + tuple((v.cpu().numpy(), nn.cpu().numpy()) for v, nn in results)
    assert H.same(got, want_pair_agg(name, expr)), (name, what)


def op_pair_agg(eng, name, log, fam, rnd):
    _pair_agg_call(eng, name, log, fam, rnd, False)


def op_pair_expr_agg(eng, name, log, fam, rnd):
    _pair_agg_call(eng, name, log, fam, rnd, True)


PAIR_AGG_OPS = [op_pair_agg, op_pair_expr_agg]      # the ``pair_agg`` family: Walk 2 and the intruders only (above)
FAMILIES = {
    "inner": [op_inner_join, op_into_exact, op_into_short, op_into_ample, op_plan_fill],
    "row": [op_semi, op_anti, op_count],
    "nearest": [op_nearest, op_nearest_k],
    "group_rows": [op_group_rows],
    "index": [op_index],
    "row_pred": [op_semi_pred, op_count_pred, op_window_join],
    "one_table": ONE_TABLE_OPS,
}
ALL_OPS = [op for fam, ops in FAMILIES.items() if fam != "row_pred" for op in ops]   # (Walk 2 and Leg 3: the seventeen)


def _check_signature(log, name):
    st = log.calls[-1][4]
    assert SIGNATURES[name](st), (name, [(k, st[k]) for k in ("sort_local", "bucket_bits", "count_fused", "join_form",
                                                                "swapped", "presorted", "n_irregular_a", "sort_resorted")])


def _check_width(log, name):
    """A settled call of a family that sorts on the tight span: the bucket width its density asks for."""
    st = log.calls[-1][4]
    if name in WIDTHS:
        assert st["sort_local"] and st["bucket_bits"] == WIDTHS[name], (name, log.calls[-1][3], st["sort_local"],
                                                                        st["bucket_bits"], st["span"])
    elif name == "sparse":
        assert not st["sort_local"], (name, log.calls[-1][3])


def _visit(eng, family, name, log):
    for rnd in (1, 2):          # 1: on the previous class's guesses; 2: on this class's own
        for op in FAMILIES[family]:
            op(eng, name, log, family, rnd)
            if family == "inner" and rnd == 2 and op is op_inner_join:
                _check_signature(log, name)
            if family in WIDTH_FAMILIES and rnd == 2:
                _check_width(log, name)


# ---------------------------------------------------------------- Walk 1
@pytest.mark.gpu
@pytest.mark.parametrize("family", list(FAMILIES))
def test_walk_every_ordered_pair_of_classes(monkeypatch, family):
    eng = _density_engine(monkeypatch)
    log = Log()
    try:
        for v in eulerian_circuit(len(NAMES)):
            _visit(eng, family, NAMES[v], log)
    finally:
        eng.close()
    pairs = log.transitions(family)
    print(f"\n[{family}] ordered class pairs covered: {len(pairs)} of {len(NAMES) ** 2}")
    assert pairs == {(x, y) for x in NAMES for y in NAMES}
    if family in WIDTH_FAMILIES:
        # the wrong-width guess was crossed: a first call on a narrow class ran the bucket stage at another width
        # than the one its settled calls took (asserted equal to WIDTHS[name] by _check_width)
        for name in ("w15", "w14", "w13"):
            firsts = [c[4] for c in log.calls if c[1] == name and c[2] == 1]
            crossed = {st["bucket_bits"] for st in firsts if st["sort_local"] and st["bucket_bits"] != WIDTHS[name]}
            print(f"[{family}] {name}: first calls ran at widths {sorted(crossed)} before settling on {WIDTHS[name]}")
            assert crossed, (family, name)
    if family == "inner":
        assert any(c[4]["bucket_join"] for c in log.calls if c[2] == 2), "no settled INNER call joined in the bucket stage"
    if family == "one_table":
        # the family reads the density guess and never sets it: this context keeps the fresh one's, every sort takes
        # four passes (a call of the family that set ``last_span`` would send w16 - w13 to the bucket stage here)
        assert not any(c[4]["sort_local"] or c[4]["sort_resorted"] for c in log.calls)
        refused = [k for k, c in enumerate(log.calls) if c[1] == "irregular" and c[3] == "cluster"]
        assert len(refused) == 2 * len(NAMES)       # each behind a refused CLUSTER of inverted rows, each right
        # coverage is one of the family in this, too ("reads the context's density guess like DISJOIN and
        # never sets it"): the operator that runs right after it -- CLUSTER of the same class, or of the next one on
        # every ordered pair of classes -- sorted in four passes (above) and was right (asserted where it ran)
        after = {(p[1], c[1]) for p, c in zip(log.calls, log.calls[1:]) if p[3] == "coverage"}
        assert all(c[3] == "cluster" for p, c in zip(log.calls, log.calls[1:]) if p[3] == "coverage")
        assert after == {(x, y) for x in NAMES for y in NAMES}, "a class pair without a call right after coverage"
        cov = [c for c in log.calls if c[3] == "coverage"]
        assert len(cov) == 2 * (len(NAMES) ** 2 + 1) and all(c[4]["span"] > 0 for c in cov)
        assert len([c for c in cov if c[1] == "irregular"]) == 2 * len(NAMES)      # each behind a refused coverage call


@pytest.mark.gpu
def test_walk_disjoin_every_ordered_pair_of_its_classes(monkeypatch):
    """The ``disjoin`` family: an Eulerian circuit over the classes on which DISJOIN's path can differ (82 visits).
    On ``irregular`` every op must raise naming the target; the visit that follows must be right."""
    eng = _density_engine(monkeypatch)
    log = Log()
    walk = eulerian_circuit(len(DISJOIN_NAMES))
    assert len(walk) == 82
    try:
        for v in walk:
            for rnd in (1, 2):
                for op in DISJOIN_OPS:
                    op(eng, DISJOIN_NAMES[v], log, "disjoin", rnd)
    finally:
        eng.close()
    pairs = log.transitions("disjoin")
    forms = sorted({(c[4]["sort_local"], c[4]["bucket_bits"]) for c in log.calls if c[1] != "irregular"})
    print(f"\n[disjoin] ordered class pairs covered: {len(pairs)} of {len(DISJOIN_NAMES) ** 2}; "
          f"(three-stage sort, bucket bits) seen: {forms}")
    assert pairs == {(x, y) for x in DISJOIN_NAMES for y in DISJOIN_NAMES}
    assert not any(c[4]["sort_resorted"] for c in log.calls)
    after = [c for p, c in zip(log.calls, log.calls[1:]) if p[1] == "irregular" and c[1] != "irregular"]
    assert len(after) == len(DISJOIN_NAMES) - 1         # every other class was visited right after the refusals


@pytest.mark.gpu
def test_walk_contain_every_ordered_pair_of_its_classes(monkeypatch):
    """The ``contain`` family: an Eulerian circuit over the classes on which CONTAINS' path can differ (65 visits) --
    the general and the uniform form, irregular rows (part X and part Y of the literal predicate),
    pile-ups of equal inner starts, many chromosomes, negative coordinates, one density that asks for narrow buckets
    and one that asks for the four global passes.  contain_plan sets the density the next call's sort form follows
    (``guess.last_span``) from its own spans, before it sorts: the settled call of a class takes the form of its own."""
    eng = _density_engine(monkeypatch)
    log = Log()
    walk = eulerian_circuit(len(CONTAIN_NAMES))
    assert len(walk) == 65
    try:
        for v in walk:
            for rnd in (1, 2):
                for op in CONTAIN_OPS:
                    op(eng, CONTAIN_NAMES[v], log, "contain", rnd)
    finally:
        eng.close()
    pairs = log.transitions("contain")
    forms = sorted({(c[1], c[4]["sort_local"], c[4]["bucket_bits"] if c[4]["sort_local"] else None) for c in log.calls},
                   key=str)
    print(f"\n[contain] ordered class pairs covered: {len(pairs)} of {len(CONTAIN_NAMES) ** 2}; "
          f"(class, three-stage sort, bucket bits) seen: {forms}")
    assert pairs == {(x, y) for x in CONTAIN_NAMES for y in CONTAIN_NAMES}
    assert not any(c[4]["sort_resorted"] for c in log.calls)
    assert {c[4]["join_form"] for c in log.calls} == {"general", "uniform_b"}
    assert all(c[4]["n_irregular_a"] + c[4]["n_irregular_b"] > 0 for c in log.calls if c[1] == "irregular")
    settled = {c[1]: c[4] for c in log.calls if c[2] == 2 and c[3] == "contains"}
    assert settled["w15"]["sort_local"] and settled["w15"]["bucket_bits"] == 15, settled["w15"]
    assert not settled["sparse"]["sort_local"]


# ---------------------------------------------------------------- Walk 2 (mixed operators, plans interrupted)
def _intrude_select(eng, name):
    _a, _b, _nch, da, _db = resident(name)
    keep = eng.select([(("a", da.start), ">=", ("lit", 0))], n=da.n, n_rows_a=da.n, want=("a",))[0].cpu().numpy()
    assert np.array_equal(keep, np.nonzero(resident(name)[0].start >= 0)[0]), (name, "select")


def _intrude_take_utf8(eng, name):
    words = [f"row{i}" * (i % 4) for i in range(300)]
    offsets = np.concatenate([[0], np.cumsum([len(w) for w in words])]).astype(np.int32)
    data = np.frombuffer("".join(words).encode(), np.uint8).copy()
    idx = np.random.default_rng(len(name)).integers(0, len(words), 5000).astype(np.int32)
    d = lambda x: torch.from_numpy(x).to("cuda:0")
    o, b = eng.take_utf8(d(offsets), d(data), d(idx))
    got = bytes(b.cpu().numpy()).decode()
    assert got == "".join(words[i] for i in idx) and o.cpu().numpy()[-1] == len(got), (name, "take_utf8")


def _intrude_inner_plan(eng, name):
    _a, _b, nch, da, db = resident(name)
    assert eng.inner_plan(da, db, nch) == want(name, "pairs").shape[0], (name, "inner_plan between a plan and its fill")


def _intrude_disjoin_plan(eng, name):
    from _disjoin_ref import plan_raw

    _a, _b, nch, da, db = resident("general")
    assert plan_raw(eng, da, db, nch) == (0, want_disjoin("general", "reference").shape[0])


def _intrude_contain_plan(eng, name):
    _a, _b, nch, da, db = resident("general")
    assert _contain_plan_raw(eng, da, db, nch) == (0, want_contain("general", "contains").shape[0])


def _intrude_one_table(op):
    """A call of the one-table family, or a pair aggregate, between a plan and its fill: every one of their entry points
    begins a call and carves the workspace anew, so whatever plan the context keeps is dropped (the columns ``cluster``,
    ``merge``, ``merge_agg``, ``merge_str``, ``coverage``, ``pair_agg`` and ``pair_expr_agg`` of
    tests/test_plan_lifetime_gpu.py: all dropped)."""
    def intruder(eng, name):
        op(eng, name, Log(), "intruder", 1)
    intruder.__name__ = "_intrude_" + op.__name__[3:]
    return intruder


INTRUDERS = {"select": _intrude_select, "take_utf8": _intrude_take_utf8, "inner_plan": _intrude_inner_plan,
             "disjoin_plan": _intrude_disjoin_plan, "contain_plan": _intrude_contain_plan, None: None,
             **{op.__name__[3:]: _intrude_one_table(op) for op in ONE_TABLE_OPS + PAIR_AGG_OPS}}
ONE_TABLE_INTRUDERS = tuple(op.__name__[3:] for op in ONE_TABLE_OPS)      # cluster, merge, merge_agg, merge_str, coverage
PAIR_AGG_INTRUDERS = tuple(op.__name__[3:] for op in PAIR_AGG_OPS)        # pair_agg, pair_expr_agg
MIXED_OPS = ALL_OPS + DISJOIN_OPS + CONTAIN_OPS + PAIR_AGG_OPS


def _which_intruder(others, turn, met):
    """What comes between the ``turn``-th plan of a kind and its fill: every third time a call of the one-table family,
    its five operators in turn (noted in ``met``); else one of ``others``, in turn."""
    if turn % 3 != 2:       # in turn, too: seven choices over the twenty such plans of a kind (a draw missed some)
        return others[(turn - turn // 3) % len(others)]
    met.append(ONE_TABLE_INTRUDERS[turn // 3 % len(ONE_TABLE_INTRUDERS)])
    return met[-1]


PLAN_OPS = {   # a plan + fill operator -> (the plan's kind, what may come between the two besides a one-table call)
    op_plan_fill: ("inner", ("select", "take_utf8", None, "disjoin_plan", "contain_plan") + PAIR_AGG_INTRUDERS),
    op_disjoin_plan_fill: ("disjoin", ("select", "take_utf8", "inner_plan", None, "contain_plan") + PAIR_AGG_INTRUDERS),
    op_contain_plan_fill: ("contain", ("select", "take_utf8", "inner_plan", "disjoin_plan", None) + PAIR_AGG_INTRUDERS),
}


@functools.lru_cache(maxsize=None)
def mixed_schedule():
    """Walk 2, call by call: ``(class, operator, what comes between its plan and its fill)`` -- every class twice, the
    operators shuffled per visit.  Pure, so that what the walk meets can be checked without a GPU."""
    r = np.random.default_rng(2027)
    visits = list(r.permutation(len(NAMES))) + list(r.permutation(len(NAMES)))
    turns = {kind: 0 for kind, _others in PLAN_OPS.values()}
    out = []
    for v in visits:
        for k in r.permutation(len(MIXED_OPS)):
            op, which = MIXED_OPS[k], None
            if op in PLAN_OPS:
                kind, others = PLAN_OPS[op]
                which = _which_intruder(others, turns[kind], [])
                turns[kind] += 1
            out.append((NAMES[v], op, which))
    return out


def interruptions(schedule):
    """plan kind -> {what interrupted it: times}.  (A DISJOIN plan on ``irregular`` is refused: nothing to interrupt.)"""
    met = {kind: {} for kind, _others in PLAN_OPS.values()}
    for name, op, which in schedule:
        if which is not None and not (op is op_disjoin_plan_fill and name == "irregular"):
            kind = PLAN_OPS[op][0]
            met[kind][which] = met[kind].get(which, 0) + 1
    return met


def test_mixed_schedule_meets_every_interruption():
    """CPU: every plan kind is interrupted by every call that can drop it -- the five one-table operators and the two
    pair aggregates among them -- and every operator runs on every class."""
    met = interruptions(mixed_schedule())
    for _kind, others in PLAN_OPS.values():
        assert all(met[_kind].get(w, 0) > 0 for w in others if w is not None), (_kind, met[_kind])
        assert all(met[_kind].get(w, 0) > 0 for w in ONE_TABLE_INTRUDERS), (_kind, met[_kind])
    assert {(name, op) for name, op, _w in mixed_schedule()} == {(name, op) for name in NAMES for op in MIXED_OPS}
    assert "coverage" in ONE_TABLE_INTRUDERS and set(PAIR_AGG_INTRUDERS) == {"pair_agg", "pair_expr_agg"}
    assert len(ALL_OPS) == 17 and len(MIXED_OPS) == 17 + 3 + 3 + 2


@pytest.mark.gpu
def test_walk_mixed_operators_with_interrupted_plans(monkeypatch):
    eng = _density_engine(monkeypatch)
    log = Log()
    try:
        for name, op, which in mixed_schedule():
            if op in PLAN_OPS:
                op(eng, name, log, "mixed", 1, intruder=INTRUDERS[which])
            else:
                op(eng, name, log, "mixed", 1)
    finally:
        eng.close()
    met = interruptions(mixed_schedule())
    interrupted = {w: met["inner"].get(w, 0) for w in ("select", "take_utf8")}
    dj_interrupted = {w: met["disjoin"].get(w, 0) for w in ("select", "take_utf8", "inner_plan", "contain_plan")}
    ct_interrupted = {w: met["contain"].get(w, 0) for w in ("select", "take_utf8", "inner_plan", "disjoin_plan")}
    inner_by_disjoin, inner_by_contain = met["inner"].get("disjoin_plan", 0), met["inner"].get("contain_plan", 0)
    by_one_table = {kind: {w: met[kind].get(w, 0) for w in ONE_TABLE_INTRUDERS} for kind in met}
    dj = [c[4] for c in log.calls if c[3].startswith("disjoin") and c[1] != "irregular"]
    forms = sorted({(st["sort_local"], st["bucket_bits"]) for st in dj})
    print(f"\n[mixed] ordered class pairs covered: {len(log.transitions('mixed'))}; interrupted plans: {interrupted}; "
          f"DISJOIN plans interrupted: {dj_interrupted}; INNER plans interrupted by a DISJOIN plan: {inner_by_disjoin}; "
          f"DISJOIN (three-stage sort, bucket bits) seen: {forms}; CONTAINS plans interrupted: {ct_interrupted}; "
          f"INNER plans interrupted by a CONTAINS plan: {inner_by_contain}; plans interrupted by a one-table call: {by_one_table}")
    assert interrupted["select"] > 0 and interrupted["take_utf8"] > 0
    assert all(v > 0 for v in dj_interrupted.values()) and inner_by_disjoin > 0
    assert all(v > 0 for v in ct_interrupted.values()) and inner_by_contain > 0
    # DISJOIN takes its bucket width from the span another operator left on the context: both sort forms were met
    assert any(st["sort_local"] for st in dj) and any(not st["sort_local"] for st in dj)
    # every plan kind was dropped by each of the five one-table operators (the refusal is asserted where it happens)
    assert all(v > 0 for kind in by_one_table.values() for v in kind.values()), by_one_table
    # ... and by both pair aggregates
    by_pair_agg = {kind: {w: met[kind].get(w, 0) for w in PAIR_AGG_INTRUDERS} for kind in met}
    print(f"[mixed] plans interrupted by a pair aggregate: {by_pair_agg}")
    assert all(v > 0 for kind in by_pair_agg.values() for v in kind.values()), by_pair_agg
    # both ran on every class, in the shuffled order (their results are asserted where they ran)
    assert {(c[1], c[3]) for c in log.calls if c[3] in PAIR_AGG_INTRUDERS} == {(x, w) for x in NAMES for w in PAIR_AGG_INTRUDERS}
    # ... which take their bucket width from the span another operator left, too: four passes and narrow buckets
    ot = [c[4] for c in log.calls if c[3] in ("cluster", "merge", "merge_agg")]
    ot_forms = sorted({(st["sort_local"], st["bucket_bits"] if st["sort_local"] else None) for st in ot}, key=str)
    print(f"[mixed] one-table (three-stage sort, bucket bits) seen: {ot_forms}")
    assert any(not st["sort_local"] for st in ot) and {st["bucket_bits"] for st in ot if st["sort_local"]} & {13, 14, 15}
    assert not any(st["sort_resorted"] for st in ot)
    # coverage sorts 2n events on the span another operator left, like DISJOIN: four passes and narrow buckets were both met
    cov = [c[4] for c in log.calls if c[3] == "coverage"]
    cov_forms = sorted({(st["sort_local"], st["bucket_bits"] if st["sort_local"] else None) for st in cov}, key=str)
    print(f"[mixed] coverage (three-stage sort, bucket bits) seen: {cov_forms}")
    assert any(not st["sort_local"] for st in cov) and {st["bucket_bits"] for st in cov if st["sort_local"]} & {13, 14, 15}
    assert not any(st["sort_resorted"] for st in cov)


# ---------------------------------------------------------------- Leg 3: the sticky four-pass fallback
@pytest.mark.gpu
def test_oversized_bucket_switches_every_context_to_four_passes_for_good(monkeypatch):
    log = Log()
    eng = None
    try:
        for x in NAMES:
            if eng is not None:
                eng.close()
            eng = _density_engine(monkeypatch)
            for _ in range(2):
                op_inner_join(eng, x, log, "settle", 1)
                op_count(eng, x, log, "settle", 1)
            for rnd in (1, 2):   # the first call decides its width from X's span, the second from its own
                op_inner_join(eng, "oversized", log, "oversized", rnd)
                op_count(eng, "oversized", log, "oversized", rnd)
            assert log.calls[-1][4]["sort_resorted"], (x, "no four-pass fallback after an oversized bucket")
        # on the last of these contexts -- today's behaviour is one-way: it stays in the four-pass sort (exact results)
        for name in NAMES:
            for op in ALL_OPS:
                op(eng, name, log, "after", 1)
                st = log.calls[-1][4]
                if op is not op_index:      # (an index is built in three stages whatever the context: index_bits)
                    assert not st["sort_local"] and st["sort_resorted"], (name, op.__name__)
    finally:
        if eng is not None:
            eng.close()


# ---------------------------------------------------------------- the 25a7a2b regression, as a walk finds it
@pytest.mark.gpu
def test_pileups_then_narrow_buckets_nearest_and_group_rows_seed_777(monkeypatch):
    """After pile-ups (NEAREST's two-sort plan), a dense table (narrow buckets): NEAREST k = 1 / k = 3 and group_rows
    must order ties by (start, end), not by input order (commit 25a7a2b, found by tools/soak.py seed 777).  The bug
    path is the two-sort plan (sticky after pile-ups) with buckets narrower than 2^16 keys: asserted on the NEAREST
    calls, so that a change of the density rules cannot quietly move this test off it.  (group_rows reports no sort
    statistics; its results are checked all the same.)"""
    for dense in ("w13", "w14"):
        for op in (op_nearest, op_nearest_k, op_group_rows):
            eng = _density_engine(monkeypatch)
            log = Log()
            try:
                op(eng, "pileups", log, "regression", 1)
                op(eng, dense, log, "regression", 1)
                op(eng, dense, log, "regression", 2)
                if op is not op_group_rows:
                    st = log.calls[-1][4]
                    assert st["sort_local"] and st["bucket_bits"] == WIDTHS[dense], (dense, op.__name__, st["bucket_bits"])
            finally:
                eng.close()


# ---------------------------------------------------------------- Leg 4: production density, default context
LEG4 = {   # name -> (reads: rows, chromosomes, axis per chromosome), the bucket width the density asks for (0: none)
    16: (3_000_000, 1, 131_000_000),         # ~1,500 rows per 65,536 keys
    15: (3_000_000, 1, 60_000_000),          # (tests/test_bucket_width.py::test_the_density_chooses_the_width)
    14: (3_000_000, 1, 30_000_000),
    13: (4_000_000, 1, 12_000_000),
    0: (3_000_000, 8, 200_000_000),          # ~120 rows per 65,536 keys: the four global passes
}


@functools.lru_cache(maxsize=None)
def leg4(bits):
    n_u, nch, span = LEG4[bits]
    reads = _rows(np.random.default_rng(4500 + bits), n_u, nch, span, 100)
    peaks = _rows(np.random.default_rng(4600 + bits), 4000, nch, span, (50, 600))
    return (peaks, reads, nch, _dev(peaks), _dev(reads), ora.sort_pairs(*ora.c_inner(peaks, reads, "sweep")),
            ora.c_nearest_k1(peaks, reads, method="sweep"))


@pytest.mark.gpu
def test_production_density_every_ordered_pair_of_widths():
    from giql_amd.engine import HipEngine

    order = list(LEG4)
    eng = HipEngine(0)
    seen = set()
    prev = None
    try:
        for v in eulerian_circuit(len(order)):
            bits = order[v]
            _peaks, reads, nch, da, db, pairs, (wi, wd) = leg4(bits)
            for rnd in (1, 2):
                ra, rb = eng.inner_join(da, db, nch)
                st = eng.stats()
                assert np.array_equal(_pairs(ra, rb), pairs), (prev, bits, rnd)
                if rnd == 2:
                    if bits:
                        assert st["sort_local"] and st["bucket_bits"] == bits and not st["sort_resorted"], (prev, bits, st)
                    else:
                        assert not st["sort_local"], (prev, bits)
                idx, dist = eng.nearest(da, db, nch)
                assert np.array_equal(dist.cpu().numpy(), wd) and _rows_equal(reads, idx.cpu().numpy(), wi), (prev, bits)
            if prev is not None:
                seen.add((prev, bits))
            prev = bits
    finally:
        eng.close()
    print(f"\n[production density] ordered width pairs covered: {len(seen)} of {len(order) ** 2}")
    assert seen == {(x, y) for x in order for y in order}
