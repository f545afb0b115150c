"""DISJOIN on the GPU: golden parity through HipEngine.disjoin and transpile + execute, seeded tables against the
brute force, the docs' recipes, skew, rejected input, empty and pinned tables, a genome wider than the 32-bit axis
and more than 2^31 output rows.  Integers throughout: every comparison is exact."""

import numpy as np
import pytest

from _disjoin_ref import OFFSETS, brute_force_arrays, golden_cases

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pa = pytest.importorskip("pyarrow")

DEV = "cuda:0"


@pytest.fixture(scope="module")
def eng():
    from giql_amd.engine import HipEngine

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    e = HipEngine(0)
    yield e
    e.close()


def _side(chrom, start, end, encoding=("0based", "half_open")):
    from giql_amd.engine import DeviceSide

    return DeviceSide.from_numpy(np.asarray(chrom, np.int32), np.asarray(start, np.int32), np.asarray(end, np.int32),
                                 encoding, device=DEV)


def _rows(parent, ds, de):
    return np.stack([parent.cpu().numpy(), ds.cpu().numpy(), de.cpu().numpy()], 1).astype(np.int64)


def _table(rows):
    return pa.table({"chrom": pa.array([r[0] for r in rows], pa.string()),
                     "start": pa.array([r[1] for r in rows], pa.int32()),
                     "end": pa.array([r[2] for r in rows], pa.int32()),
                     "name": pa.array([r[3] for r in rows], pa.string())})


CASES = golden_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_golden_engine(eng, case):
    names = sorted({r[0] for r in case["target"]} | {r[0] for r in case["reference"] or []})
    code = {n: i for i, n in enumerate(names)}
    t = case["target"]
    target = _side([code[r[0]] for r in t], [r[1] for r in t], [r[2] for r in t], tuple(case["encoding"]))
    reference = None
    if case["reference"] is not None:
        r = case["reference"]
        reference = _side([code[x[0]] for x in r], [x[1] for x in r], [x[2] for x in r])
    got = _rows(*eng.disjoin(target, reference, len(names)))
    assert got.tolist() == case["expected"]          # ordered by parent, then start: the fixture's sorted order


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_golden_execute(eng, case):
    from giql_amd.execute import execute
    from giql_amd.table import Table
    from giql_amd.transpile import transpile

    cs, it = case["encoding"]
    tables = [Table("features", coordinate_system=cs, interval_type=it), "refs"]
    data = {"features": _table(case["target"])}
    query = "SELECT * FROM DISJOIN(features)"
    if case["reference"] is not None:
        data["refs"] = _table(case["reference"])
        query = "SELECT * FROM DISJOIN(features, reference := refs)"
    out = execute(transpile(query, tables, dialect="hip"), data, eng)
    assert out.column_names == ["chrom", "start", "end", "name", "disjoin_chrom", "disjoin_start", "disjoin_end"]
    got = sorted(zip(*(out.column(n).to_pylist() for n in out.column_names)))
    t = case["target"]
    want = sorted((t[p][0], t[p][1], t[p][2], t[p][3], t[p][0], s, e) for p, s, e in case["expected"])
    assert got == want
    idx = execute(transpile(query, tables, dialect="hip"), data, eng, return_indices=True)
    assert sorted(map(list, zip(*(x.tolist() for x in idx)))) == case["expected"]


def _random_table(rng, n, n_chrom, top, max_len, points=0.02):
    chrom = rng.integers(0, n_chrom, n)
    start = rng.integers(0, top, n)
    length = rng.integers(1, max_len, n)
    length[rng.random(n) < points] = 0
    return chrom.astype(np.int64), start.astype(np.int64), (start + length).astype(np.int64)


@pytest.mark.parametrize("n_t, n_r", [(1_000, 0), (1_000, 3_000), (100_000, 0), (30_000, 100_000)])
def test_seeded_random_against_brute_force(eng, n_t, n_r):
    rng = np.random.default_rng(1000 + n_t + n_r)
    tc, ts, te = _random_table(rng, n_t, 24, 2_000_000, 5_000)
    reference, ref_np = None, ()
    if n_r:
        rc, rs, re_ = _random_table(rng, n_r, 24, 2_000_000, 400)   # sparse enough to leave uncovered gaps
        reference, ref_np = _side(rc, rs, re_), (rc, rs, re_)
    got = _rows(*eng.disjoin(_side(tc, ts, te), reference, 24))
    want = brute_force_arrays(tc, ts, te, *ref_np)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert eng.stats()["n_out"] == len(want)


def test_docs_recipes(eng):
    from giql_amd.execute import execute

    feats = _table([("chr1", 0, 20, "A"), ("chr1", 10, 30, "B"), ("chr2", 5, 25, "C")])
    out = execute("SELECT DISTINCT disjoin_chrom, disjoin_start, disjoin_end FROM DISJOIN(features) ORDER BY disjoin_start",
                  {"features": feats}, eng, giql_tables=["features"])
    assert list(zip(*(out.column(n).to_pylist() for n in out.column_names))) == [
        ("chr1", 0, 10), ("chr2", 5, 25), ("chr1", 10, 20), ("chr1", 20, 30)]
    # re-tile against a uniform grid: every feature cut at the bin edges, each piece inside one bin
    bins = _table([("chr1", k, k + 8, f"bin{k}") for k in range(0, 40, 8)] + [("chr2", k, k + 8, f"bin{k}") for k in range(0, 40, 8)])
    out = execute("SELECT name, disjoin_start, disjoin_end FROM DISJOIN(features, reference := bins) ORDER BY name, disjoin_start",
                  {"features": feats, "bins": bins}, eng, giql_tables=["features", "bins"])
    assert list(zip(*(out.column(n).to_pylist() for n in out.column_names))) == [
        ("A", 0, 8), ("A", 8, 16), ("A", 16, 20), ("B", 10, 16), ("B", 16, 24), ("B", 24, 30),
        ("C", 5, 8), ("C", 8, 16), ("C", 16, 24), ("C", 24, 25)]


def test_skew_one_chromosome_long_target(eng):
    """One target over a whole chromosome against 1.2M reference rows (a gap-free grid of 10-base rows), beside 1e5
    short targets: closed form -- a target [s, e) inside the grid leaves ceil(e / 10) - floor(s / 10) pieces."""
    n_ref, step = 1_200_000, 10
    rs = np.arange(n_ref, dtype=np.int64) * step
    rng = np.random.default_rng(7)
    ts = np.concatenate([[0], rng.integers(0, n_ref * step - 200, 100_000)])
    te = np.concatenate([[n_ref * step], ts[1:] + rng.integers(1, 200, 100_000)])
    zeros = np.zeros(len(ts), np.int64)
    parent, ds, de = eng.disjoin(_side(zeros, ts, te), _side(np.zeros(n_ref), rs, rs + step), 1)
    counts = (te + step - 1) // step - ts // step
    assert int(parent.shape[0]) == int(counts.sum())
    assert np.array_equal(torch.bincount(parent.long(), minlength=len(ts)).cpu().numpy(), counts)
    # the long row: its pieces are the grid itself
    k = torch.arange(n_ref, device=DEV, dtype=torch.int32) * step
    assert torch.equal(ds[:n_ref], k) and torch.equal(de[:n_ref], k + step) and int(parent[:n_ref].max()) == 0
    # every piece lies inside its parent and inside one grid cell; per parent the pieces tile [s, e)
    ps, pe = torch.as_tensor(ts, device=DEV)[parent.long()], torch.as_tensor(te, device=DEV)[parent.long()]
    assert bool(((ds >= ps) & (de <= pe) & (ds < de) & (torch.div(ds, step, rounding_mode="floor") ==
                                                       torch.div(de - 1, step, rounding_mode="floor"))).all())
    length = torch.zeros(len(ts), dtype=torch.int64, device=DEV).index_add_(0, parent.long(), (de - ds).long())
    assert np.array_equal(length.cpu().numpy(), te - ts)
    sample = rng.integers(1, len(ts), 200)
    want = brute_force_arrays(zeros[sample], ts[sample], te[sample], np.zeros(n_ref, np.int64), rs, rs + step)
    got = _rows(parent, ds, de)
    sel = got[np.isin(got[:, 0], sample)]
    remap = {int(p): i for i, p in enumerate(sample)}
    # (sample rows may repeat: compare per sampled parent)
    for i, p in enumerate(sample):
        assert np.array_equal(sel[sel[:, 0] == p][:, 1:], want[want[:, 0] == i][:, 1:])
    assert remap


def test_start_after_end_is_rejected_naming_the_side(eng):
    from giql_amd.execute import execute

    good = _side([0, 0], [0, 10], [20, 30])
    bad = _side([0, 0], [0, 30], [20, 10])
    with pytest.raises(ValueError, match="target"):
        eng.disjoin(bad, None, 1)
    with pytest.raises(ValueError, match="target"):
        eng.disjoin(bad, good, 1)
    with pytest.raises(ValueError, match="reference"):
        eng.disjoin(good, bad, 1)
    feats, refs = _table([("chr1", 0, 20, "A")]), _table([("chr1", 30, 10, "r")])
    with pytest.raises(ValueError, match="'refs'"):
        execute("SELECT * FROM DISJOIN(features, reference := refs)", {"features": feats, "refs": refs}, eng,
                giql_tables=["features", "refs"])
    with pytest.raises(ValueError, match="'refs'"):
        execute("SELECT * FROM DISJOIN(refs)", {"refs": refs}, eng, giql_tables=["refs"])
    assert _rows(*eng.disjoin(good, None, 1)).tolist() == [[0, 0, 10], [0, 10, 20], [1, 10, 20], [1, 20, 30]]


def test_empty_sides_and_pinned_reference(eng):
    from giql_amd import pin
    from giql_amd.execute import execute

    some = _side([0, 1], [0, 5], [20, 25])
    empty = _side([], [], [])
    assert all(int(t.shape[0]) == 0 for t in eng.disjoin(empty, None, 2))
    assert all(int(t.shape[0]) == 0 for t in eng.disjoin(empty, some, 2))
    assert all(int(t.shape[0]) == 0 for t in eng.disjoin(some, empty, 2))       # nothing is covered
    assert all(int(t.shape[0]) == 0 for t in eng.disjoin(_side([0], [0], [9]), _side([1], [0], [9]), 2))
    feats, other = _table([("chr1", 0, 30, "T")]), _table([("chr1", 5, 12, "U"), ("chr2", 0, 9, "V")])
    refs = pin(_table([("chr1", 0, 10, "a"), ("chr1", 20, 30, "b")]))
    try:
        q = "SELECT name, disjoin_start, disjoin_end FROM DISJOIN({}, reference := refs) ORDER BY disjoin_start"
        one = execute(q.format("features"), {"features": feats, "refs": refs}, eng, giql_tables=["features", "refs"])
        two = execute(q.format("other"), {"other": other, "refs": refs}, eng, giql_tables=["other", "refs"])
    finally:
        refs.unpin()
    assert list(zip(*(one.column(n).to_pylist() for n in one.column_names))) == [("T", 0, 10), ("T", 20, 30)]
    assert list(zip(*(two.column(n).to_pylist() for n in two.column_names))) == [("U", 5, 10)]
    empty_out = execute("SELECT * FROM DISJOIN(features)", {"features": _table([])}, eng, giql_tables=["features"])
    assert empty_out.num_rows == 0 and empty_out.column_names[-3:] == ["disjoin_chrom", "disjoin_start", "disjoin_end"]


def test_genome_wider_than_the_axis_falls_back_by_chromosome_group(eng):
    """Three chromosomes of 2e9 bases each: their spans sum past 2^32, the call reports GIQL_ERR_SPAN and the engine
    runs the chromosome groups one by one."""
    from giql_amd import _lib

    rng = np.random.default_rng(3)
    far = 2_000_000_000
    tc = rng.integers(0, 3, 3_000).astype(np.int64)
    ts = np.where(rng.random(3_000) < 0.5, rng.integers(0, 5_000, 3_000), far + rng.integers(0, 5_000, 3_000))
    te = ts + rng.integers(0, 300, 3_000)
    rc = rng.integers(0, 3, 5_000).astype(np.int64)
    rs = np.where(rng.random(5_000) < 0.5, rng.integers(0, 5_000, 5_000), far + rng.integers(0, 5_000, 5_000))
    re_ = rs + rng.integers(0, 60, 5_000)
    target, reference = _side(tc, ts, te), _side(rc, rs, re_)
    with pytest.raises(_lib.GiqlHipError) as ei:
        eng._disjoin_once(target, reference, 3)
    assert ei.value.code == _lib.GIQL_ERR_SPAN
    assert np.array_equal(_rows(*eng.disjoin(target, reference, 3)), brute_force_arrays(tc, ts, te, rc, rs, re_))
    assert np.array_equal(_rows(*eng.disjoin(target, None, 3)), brute_force_arrays(tc, ts, te))


def test_more_than_2_31_output_rows(eng):
    """40,000 identical targets [0, 600000) over a gap-free grid of 60,000 ten-base reference rows: 2.4e9 rows
    (29 GB of int32 outputs).  Closed form: slot k belongs to parent k // 60000 and is piece (k % 60000) of the grid."""
    n_t, n_grid, step = 40_000, 60_000, 10
    total = n_t * n_grid
    assert total > 2**31
    free = torch.cuda.mem_get_info(0)[0]
    if free < 3 * 4 * total + (24 << 30):
        pytest.skip(f"needs {(3 * 4 * total + (24 << 30)) >> 30} GiB of free HBM, {free >> 30} GiB are free")
    rs = np.arange(n_grid, dtype=np.int64) * step
    target = _side(np.zeros(n_t), np.zeros(n_t), np.full(n_t, n_grid * step))
    parent, ds, de = eng.disjoin(target, _side(np.zeros(n_grid), rs, rs + step), 1)
    assert int(parent.shape[0]) == total == eng.stats()["n_out"]
    chunk = 1 << 28
    for k0 in range(0, total, chunk):
        k = torch.arange(k0, min(k0 + chunk, total), device=DEV, dtype=torch.int64)
        sl = slice(k0, min(k0 + chunk, total))
        assert torch.equal(parent[sl].long(), k // n_grid), k0       # per-parent counts: every parent owns n_grid slots
        piece = (k % n_grid) * step
        assert torch.equal(ds[sl].long(), piece) and torch.equal(de[sl].long(), piece + step), k0
        del k, piece
    for p in (0, 1, n_t // 2, n_t - 1):                                # first and last piece of a sample of parents
        a, b = p * n_grid, (p + 1) * n_grid - 1
        assert (int(parent[a]), int(ds[a]), int(de[a])) == (p, 0, step)
        assert (int(parent[b]), int(ds[b]), int(de[b])) == (p, (n_grid - 1) * step, n_grid * step)
