"""Coverage depth per DISJOIN segment on the GPU: ``giql_hip_coverage_dev`` / ``HipEngine.coverage`` and the three
query forms of ``disjoin_aggregates=True`` through ``execute()`` -- needs a GPU.

Every comparison is exact (integers throughout).  The references are tests/_coverage_ref.py's, held on the CPU
(tests/test_coverage.py) to each other, to DISJOIN's sqlite-minted pieces grouped by segment and to the sqlite-minted
tests/golden/coverage.json.  Sizes: 2n events straddle a 256-thread block at n = 128, the 4,096-element scan tile at
n = 2,048 and the 8,192-event sort tile at n = 4,096; 20,001 rows take several of each."""

import numpy as np
import pytest

import _coverage_queries as Q
import _coverage_ref as R
import _disjoin_ref as D
import _stream_harness as H
from test_axis_edges import LAYOUTS, TOP, dev as edge_dev, make_side, tight_span
from test_disjoin_paths import FORMS, _assert_form, _engine

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
SENTINEL = -77
HALF_OPEN = ("0based", "half_open")


@pytest.fixture(scope="module")
def eng():
    e = _engine({})
    yield e
    e.close()


def _side(cols, enc=HALF_OPEN):
    from giql_amd.engine import DeviceSide

    return DeviceSide.from_numpy(*(np.asarray(x, np.int32) for x in cols), enc, device=DEV)


def _rows(out):
    """The engine's four tensors as an int64 array [m, 4] (or [m, 3] without the depth)."""
    return np.stack([t.cpu().numpy().astype(np.int64) for t in out if t is not None], 1)


def _check(eng, cols, n_chrom, enc=HALF_OPEN, what=None):
    """Depth, runs and no-depth forms of one table against the vectorised reference."""
    side = _side(cols, enc)
    for runs in (False, True):
        want = R.sweep_arrays(*cols, enc, runs=runs)
        out = eng.coverage(side, n_chrom, runs=runs)
        assert [t.dtype for t in out] == [torch.int32, torch.int32, torch.int32, torch.int64]
        got = _rows(out)
        assert got.shape == want.shape and np.array_equal(got, want), (what, runs)
        assert eng.stats()["n_out"] == len(want)
        bare = eng.coverage(side, n_chrom, runs=runs, with_depth=False)
        assert bare[3] is None and np.array_equal(_rows(bare), want[:, :3]), (what, runs, "no depth")


# ---------------------------------------------------------------- goldens
def _golden_columns(rows):
    names = sorted({r[0] for r in rows})
    cols = [np.array([names.index(r[0]) for r in rows], np.int64), np.array([r[1] for r in rows], np.int64),
            np.array([r[2] for r in rows], np.int64)]
    return names, cols


@pytest.mark.parametrize("case", R.golden_cases(), ids=lambda c: c["id"])
def test_sqlite_minted_coverage(eng, case):
    names, cols = _golden_columns(case["rows"])
    enc = tuple(case["encoding"])
    side = _side(cols, enc)
    ids = lambda rows: np.array([[names.index(r[0])] + list(r[1:]) for r in rows], np.int64).reshape(-1, 4)  # noqa: E731
    assert np.array_equal(_rows(eng.coverage(side, len(names))), ids(case["segments"]))
    assert np.array_equal(_rows(eng.coverage(side, len(names), with_depth=False)), ids(case["segments"])[:, :3])
    if case["runs"] is not None:
        assert np.array_equal(_rows(eng.coverage(side, len(names), runs=True)), ids(case["runs"]))
        assert np.array_equal(_rows(eng.coverage(side, len(names), runs=True, with_depth=False)), ids(case["runs"])[:, :3])
    else:   # the kernel merges by canonical abutment; only the SQL recipe declines a closed target
        assert np.array_equal(_rows(eng.coverage(side, len(names), runs=True)), R.sweep_arrays(*cols, enc, runs=True))


SELF_CASES = [c for c in D.golden_cases() if c["reference"] is None]


@pytest.mark.parametrize("case", SELF_CASES, ids=lambda c: c["id"])
def test_disjoin_goldens_grouped_by_segment(eng, case):
    names, cols = _golden_columns(case["target"])
    want = np.array(R.group_pieces(cols[0].tolist(), case["expected"]), np.int64).reshape(-1, 4)
    side = _side(cols, tuple(case["encoding"]))
    assert np.array_equal(_rows(eng.coverage(side, len(names))), want)
    assert np.array_equal(_rows(eng.coverage(side, len(names), with_depth=False)), want[:, :3])
    assert np.array_equal(_rows(eng.coverage(side, len(names), runs=True)),
                          R.sweep_arrays(*cols, tuple(case["encoding"]), runs=True))


# ---------------------------------------------------------------- edges of the machinery
SIZES = (0, 1, 2, 127, 128, 129, 2047, 2048, 2049, 4095, 4096, 4097, 20_001)


@pytest.mark.parametrize("n", SIZES)
def test_every_shape_at_every_edge_size(eng, n):
    for kind in R.SHAPES:
        _check(eng, R.shaped_table(kind, n), 1, what=(kind, n))


def test_no_rows_is_ok_without_a_dictionary(eng):
    z = np.zeros(0, np.int64)
    for n_chrom in (0, 3):
        out = eng.coverage(_side((z, z, z)), n_chrom)
        assert [int(t.numel()) for t in out] == [0, 0, 0, 0] and eng.stats()["n_out"] == 0


def test_deep_pile_keeps_a_depth_past_16_bits(eng):
    n = 70_000
    cols = (np.zeros(n + 1, np.int64), np.concatenate([np.full(n, 500), [100]]), np.concatenate([np.full(n, 900), [2000]]))
    want = np.array([[0, 100, 500, 1], [0, 500, 900, n + 1], [0, 900, 2000, 1]], np.int64)
    assert np.array_equal(R.sweep_arrays(*cols), want)
    _check(eng, cols, 1, what="deep pile")
    assert np.array_equal(_rows(eng.coverage(_side(cols), 1)), want)


# ---------------------------------------------------------------- chromosomes
def test_300_chromosomes_with_one_row_each(eng):
    c = np.arange(300, dtype=np.int64)
    cols = (c[::-1].copy(), 1000 - c, 1000 - c + 1 + c % 7)
    _check(eng, cols, 300, what="300 chromosomes")
    assert len(R.sweep_arrays(*cols, runs=True)) == 300


def test_chromosomes_without_a_row_at_the_front_in_the_middle_and_at_the_end(eng):
    cols = (np.array([1, 2, 4, 4, 1], np.int64), np.array([10, 0, 5, 8, 10], np.int64), np.array([20, 7, 9, 30, 15], np.int64))
    _check(eng, cols, 6, what="empty chromosomes")
    assert set(R.sweep_arrays(*cols)[:, 0].tolist()) == {1, 2, 4}


def test_nothing_merges_across_a_chromosome_boundary(eng):
    """Rows ending exactly where the next chromosome's first row begins in raw coordinates, with equal depth."""
    c = np.repeat(np.arange(5, dtype=np.int64), 2)
    s = np.repeat(100 * np.arange(5, dtype=np.int64), 2)
    cols = (c, s, s + 100)                                    # chromosome k: two copies of [100k, 100k + 100)
    want = np.array([[k, 100 * k, 100 * k + 100, 2] for k in range(5)], np.int64)
    assert np.array_equal(R.sweep_arrays(*cols, runs=True), want)
    _check(eng, cols, 5, what="abutting across chromosomes")
    assert np.array_equal(_rows(eng.coverage(_side(cols), 5, runs=True)), want)


# ---------------------------------------------------------------- axis ends, encodings, the wide genome
def _edge_want(t, enc, runs):
    return R.sweep_arrays(t.chrom.astype(np.int64), t.start.astype(np.int64), t.end.astype(np.int64), enc, runs=runs)


@pytest.mark.parametrize("enc", [("0based", "half_open"), ("1based", "closed")], ids=lambda e: e[0])
@pytest.mark.parametrize("name", ["tight_top", "one_chrom_max"])
def test_keys_at_zero_and_at_the_top_of_the_axis(eng, name, enc):
    t = make_side(name, enc, 2500, 18, zero_length=True)
    if name == "tight_top":
        key = t.ce[t.chrom == 1].astype(np.int64) + 2**31 - 1
        assert key.max() == TOP - 1 and t.cs[t.chrom == 0].min() == 0
    for runs in (False, True):
        got = _rows(eng._coverage_once(edge_dev(t), len(LAYOUTS[name]), runs, True))
        assert eng.stats()["span"] == tight_span(name)
        want = _edge_want(t, enc, runs)
        assert len(want) > 1000 and got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("enc", list(D.OFFSETS), ids=lambda e: "-".join(e))
def test_all_four_encodings(eng, enc):
    so, eo = D.OFFSETS[enc]
    for seed in range(6):
        c, s, e, n_chrom = R.seeded_table(seed)
        _check(eng, (c, s - so, e - eo), n_chrom, enc, what=(enc, seed))     # closed ones through runs=True as well


def test_wide_genome_falls_back_to_chromosome_groups(eng):
    from giql_amd import _lib

    enc = ("1based", "closed")
    t = make_side("tight_over", enc, 2500, 21, zero_length=True)             # two chromosomes, spans summing to 2^32
    assert tight_span("tight_over") == 2**32
    with pytest.raises(_lib.GiqlHipError) as ei:
        eng._coverage_once(edge_dev(t), 2, False, True)
    assert ei.value.code == _lib.GIQL_ERR_SPAN
    for runs in (False, True):
        got = _rows(eng.coverage(edge_dev(t), 2, runs=runs))
        assert np.array_equal(got, _edge_want(t, enc, runs))
        bare = eng.coverage(edge_dev(t), 2, runs=runs, with_depth=False)
        assert bare[3] is None and np.array_equal(_rows(bare), _edge_want(t, enc, runs)[:, :3])


# ---------------------------------------------------------------- sort forms
FORM_TABLES = ("distinct", "chain", "alternating", "nested", "points-inside")


@pytest.mark.parametrize("form", list(FORMS))
def test_under_every_sort_form(form):
    e = _engine(FORMS[form][0])
    e.form = form
    try:
        for kind in FORM_TABLES:
            cols = R.shaped_table(kind, 4097)
            for runs in (False, True):
                got = _rows(e.coverage(_side(cols), 1, runs=runs))
                assert np.array_equal(got, R.sweep_arrays(*cols, runs=runs)), (form, kind, runs)
                _assert_form(e)
    finally:
        e.close()


# ---------------------------------------------------------------- calling conventions
def _sentinels(n):
    return [torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV) for _ in range(3)] + \
        [torch.full((n,), SENTINEL, dtype=torch.int64, device=DEV)]


@pytest.mark.parametrize("flags", [0, 1])
def test_capacity_one_short_reports_the_need_and_writes_nothing(eng, flags):
    from giql_amd import _lib

    cols = R.shaped_table("alternating", 129)
    want = R.sweep_arrays(*cols, runs=bool(flags))
    outs = _sentinels(len(want) + 8)
    rc, n = R.coverage_raw(eng, _side(cols), 1, flags, outs, len(want) - 1)
    assert rc == _lib.GIQL_ERR_CAPACITY and n == len(want)
    assert all(bool((o == SENTINEL).all()) for o in outs)
    rc, n = R.coverage_raw(eng, _side(cols), 1, flags, outs, len(want))
    assert rc == _lib.GIQL_OK and n == len(want) and eng.stats()["n_out"] == len(want)
    assert np.array_equal(np.stack([o[:n].cpu().numpy().astype(np.int64) for o in outs], 1), want)
    assert all(bool((o[n:] == SENTINEL).all()) for o in outs)


def test_bad_arguments_are_refused(eng):
    from giql_amd import _lib

    some = _side(([0], [0], [9]))
    outs = _sentinels(4)
    assert R.coverage_raw(eng, some, 1, 2, outs, 4)[0] == _lib.GIQL_ERR_INVALID          # unknown flag
    assert R.coverage_raw(eng, some, -1, 0, outs, 4)[0] == _lib.GIQL_ERR_INVALID
    assert R.coverage_raw(eng, some, 0, 0, outs, 4) == (_lib.GIQL_ERR_CHROM, 0)
    assert R.coverage_raw(eng, some, 1, 0, [None, outs[1], outs[2], outs[3]], 4)[0] == _lib.GIQL_ERR_INVALID
    assert all(bool((o == SENTINEL).all()) for o in outs)
    assert R.coverage_raw(eng, some, 1, 0, outs[:3] + [None], 4) == (_lib.GIQL_OK, 1)     # depth_out may be NULL
    assert [int(o[0]) for o in outs[:3]] == [0, 0, 9] and int(outs[3][0]) == SENTINEL


def test_start_after_end_is_a_value_error(eng):
    bad = _side(([0, 0, 0], [0, 30, 5], [20, 10, 9]))
    for runs in (False, True):
        with pytest.raises(ValueError, match="start > end"):
            eng.coverage(bad, 1, runs=runs)
    _check(eng, R.shaped_table("nested", 50), 1, what="after the error")


def test_the_call_drops_a_kept_inner_plan_and_a_kept_disjoin_plan(eng):
    from giql_amd import _lib

    a = _side(R.shaped_table("nested", 300))
    b = _side(R.shaped_table("chain", 300))
    n = eng.inner_plan(a, b, 1)
    assert n > 0
    eng.coverage(b, 1)
    ra, rb = (torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV) for _ in range(2))
    with pytest.raises(_lib.GiqlHipError) as ei:
        eng.inner_fill(ra, rb)
    assert ei.value.code == _lib.GIQL_ERR_STATE and bool((ra == SENTINEL).all())
    rc, pieces = D.plan_raw(eng, a, None, 1)
    assert rc == 0 and pieces > 0
    eng.coverage(b, 1, runs=True)
    outs = [torch.full((pieces,), SENTINEL, dtype=torch.int32, device=DEV) for _ in range(3)]
    assert D.fill_raw(eng, outs, pieces) == _lib.GIQL_ERR_STATE
    assert all(bool((o == SENTINEL).all()) for o in outs)


def test_on_a_side_stream_behind_pending_work(eng):
    """The stale / fresh protocol of tests/_stream_harness.py: the table is rewritten on a side stream behind a delay
    just before the call and back right after it.  A launch on another stream would read the stale rows."""
    be = H.TorchBackend()
    s = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        torch.cuda._sleep(1000)
        e0.record()
        torch.cuda._sleep(2_000_000)
        e1.record()
    s.synchronize()
    cycles = int(2_000_000 / max(e0.elapsed_time(e1), 1e-3) * 25)        # about 25 ms
    make = H.one_table(5000, 5)
    stale, fresh = make(H.STALE_SEED), make(H.FRESH_SEED)
    cols = lambda inp: tuple(inp[f"a.{k}"].astype(np.int64) for k in ("chrom", "start", "end"))  # noqa: E731
    bystander = torch.arange(4096, device=DEV)                            # the default stream's data
    torch.cuda.synchronize()
    for runs in (False, True):
        want_fresh, want_stale = R.sweep_arrays(*cols(fresh), runs=runs), R.sweep_arrays(*cols(stale), runs=runs)
        assert want_fresh.shape != want_stale.shape or not np.array_equal(want_fresh, want_stale)
        out, clones = H.run_protocol(be, s, stale, fresh, lambda bufs: eng.coverage(H.dside(bufs, "a"), 5, runs=runs),
                                     cycles)
        got = np.stack([np.asarray(x).astype(np.int64) for x in out], 1)
        assert got.shape == want_fresh.shape and np.array_equal(got, want_fresh), runs
        assert all(np.array_equal(clones[k], fresh[k]) for k in fresh)     # the inputs as the call found them
    assert torch.equal(bystander, torch.arange(4096, device=DEV))


# ---------------------------------------------------------------- execute()
def _arrow(cols, names):
    import pyarrow as pa

    return pa.table({"chrom": pa.array([names[c] for c in cols[0].tolist()]), "start": pa.array(cols[1], type=pa.int32()),
                     "end": pa.array(cols[2], type=pa.int32()), "name": pa.array([f"r{i}" for i in range(len(cols[0]))])})


def _multi_chrom_table(n, seed):
    r = np.random.default_rng(seed)
    c = r.integers(0, 4, n)
    s = r.integers(0, 3000, n) * 5
    return c.astype(np.int64), s.astype(np.int64), (s + r.integers(0, 40, n) * 5).astype(np.int64)


NAMES = ["chr1", "chr10", "chr2", "chrX"]          # sorted as strings: the dictionary's order


def test_execute_the_three_query_forms(eng):
    from giql_amd.execute import execute

    cols = _multi_chrom_table(800, 5)
    tables = {"features": _arrow(cols, NAMES)}
    seg, runs = R.sweep_arrays(*cols), R.sweep_arrays(*cols, runs=True)
    run = lambda q, **kw: execute(q, tables, eng, giql_tables=Q.TABLES, disjoin_aggregates=True, **kw)  # noqa: E731

    out = run(Q.DEPTH)
    assert out.column_names == ["chrom", "start", "end", "depth"]
    assert [str(t) for t in out.schema.types] == ["string", "int32", "int32", "int64"]
    got = sorted(zip(*(out.column(k).to_pylist() for k in out.column_names)))
    assert got == sorted((NAMES[c], s, e, d) for c, s, e, d in seg.tolist())

    top = run(Q.DEPTH + " ORDER BY depth DESC, chrom, start LIMIT 3")
    want = sorted(((-d, NAMES[c], s, e) for c, s, e, d in seg.tolist()))[:3]
    assert list(zip(*(top.column(k).to_pylist() for k in ("depth", "chrom", "start", "end")))) == \
        [(-d, c, s, e) for d, c, s, e in want]

    aliased = run("SELECT d.disjoin_end AS e, COUNT(*) AS n, d.disjoin_chrom AS c FROM DISJOIN(features) AS d "
                  "GROUP BY d.disjoin_start, d.disjoin_end, d.disjoin_chrom ORDER BY disjoin_start, c")
    assert aliased.column_names == ["e", "n", "c"]
    by_start = sorted(seg.tolist(), key=lambda r: (r[1], NAMES[r[0]]))
    assert aliased.column("e").to_pylist() == [r[2] for r in by_start]
    assert aliased.column("n").to_pylist() == [r[3] for r in by_start]

    dist = run(Q.ACCEPTED["distinct_recipe"][0])
    assert dist.column_names == ["disjoin_chrom", "disjoin_start", "disjoin_end"]
    assert sorted(zip(*(dist.column(k).to_pylist() for k in dist.column_names))) == \
        sorted((NAMES[c], s, e) for c, s, e, _d in seg.tolist())

    merged = run(Q.RUNS + " ORDER BY chrom, start")
    assert merged.column_names == ["chrom", "start", "end"]
    assert list(zip(*(merged.column(k).to_pylist() for k in merged.column_names))) == \
        sorted((NAMES[c], s, e) for c, s, e, _d in runs.tolist())

    for query, want, depth in ((Q.DEPTH, seg, True), (Q.RUNS, runs, True), (Q.ACCEPTED["distinct_recipe"][0], seg, False)):
        c, s, e, d = run(query, return_indices=True)
        assert all(isinstance(x, np.ndarray) for x in (c, s, e)) and (d is None) != depth
        assert np.array_equal(np.stack([c, s, e], 1).astype(np.int64), want[:, :3])
        assert not depth or (d.dtype == np.int64 and np.array_equal(d, want[:, 3]))


def test_execute_names_the_table_with_a_bad_row(eng):
    from giql_amd.execute import execute

    cols = (np.zeros(3, np.int64), np.array([0, 30, 5], np.int64), np.array([20, 10, 9], np.int64))
    with pytest.raises(ValueError, match=r"table 'features' has a row with start > end"):
        execute(Q.DEPTH, {"features": _arrow(cols, NAMES)}, eng, giql_tables=Q.TABLES, disjoin_aggregates=True)


@pytest.mark.parametrize("table", ["features", "open1"])
def test_execute_the_run_recipe_against_the_sqlite_minted_runs(eng, table):
    from giql_amd.execute import execute

    enc = ["0based" if table == "features" else "1based", "half_open"]
    cases = [c for c in R.golden_cases() if c["encoding"] == enc]
    assert len(cases) == 15
    for case in cases:
        names, cols = _golden_columns(case["rows"])
        tables = {table: _arrow(cols, names)}
        for query, key in ((Q.RUNS, "runs"), (Q.DEPTH, "segments")):
            out = execute(query.replace("features", table) + " ORDER BY chrom, start", tables, eng, giql_tables=Q.TABLES,
                          disjoin_aggregates=True)
            got = [list(r) for r in zip(*(out.column(k).to_pylist() for k in out.column_names))]
            assert got == [r[:len(out.column_names)] for r in case[key]], (case["id"], key)


def test_distinct_recipe_with_and_without_the_flag_on_one_context(eng):
    from giql_amd.execute import execute

    cols = _multi_chrom_table(5000, 9)
    tables = {"features": _arrow(cols, NAMES)}
    query = Q.ACCEPTED["distinct_recipe"][0]
    new = execute(query, tables, eng, giql_tables=Q.TABLES, disjoin_aggregates=True)
    old = execute(query, tables, eng, giql_tables=Q.TABLES)
    assert new.column_names == old.column_names and [str(t) for t in new.schema.types][1:] == ["int32", "int32"]
    rows = lambda t: sorted(zip(*(t.column(k).to_pylist() for k in t.column_names)))  # noqa: E731
    assert rows(new) == rows(old) and len(rows(new)) == len(R.sweep_arrays(*cols)) > 1000
