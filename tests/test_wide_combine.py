"""The combiners of ``giql_amd/wide.py`` on CPU tensors, against the oracle -- no GPU.

``HipEngine._wide`` answers a genome wider than the 32-bit axis chromosome group by chromosome group and hands the
groups' results to a combiner.  Here two small tables are split by hand into the groups ``GROUPS``, the oracle runs
on each group's sub-tables in place of the GPU call, the function under test combines, and the result must equal the
oracle's on the whole tables.  Chromosome 1 holds rows of A only (its group's B is empty), chromosome 2 rows of B
only.  The same path on the GPU: tests/test_axis_edges.py.
"""

import numpy as np
import pytest

import _contain_ref as C
import _disjoin_ref as D
import _distance_ref as W
from oracle import pyoracle as ora

torch = pytest.importorskip("torch")

from giql_amd import wide  # noqa: E402

GROUPS = [[0, 3], [1], [2]]
CPU = torch.device("cpu")


def table(seed, n, chroms, enc):
    """``n`` rows on ``chroms`` below 100,000, a dense corner so that rows meet, zero-length rows, and a quarter of
    the rows copies of earlier ones (equal keys within a chromosome, equal coordinates across chromosomes)."""
    r = np.random.default_rng(seed)
    so, eo = ora.ENCODING_OFFSETS[enc]
    ch = np.asarray(chroms)[r.integers(0, len(chroms), n)]
    cs = np.where(r.random(n) < 0.6, r.integers(0, 4000, n), r.integers(0, 99_000, n))
    ce = cs + np.where(r.random(n) < 0.05, 0, r.integers(1, 400, n))
    dup = np.arange(n - n // 4, n)
    src = r.integers(0, n - n // 4, dup.size)
    cs[dup], ce[dup] = cs[src], ce[src]
    ch[dup[::2]] = ch[src[::2]]
    return ora.Side(ch, cs - so, ce - eo, so, eo)


A = table(1, 200, [0, 1, 3], ("1based", "closed"))
B = table(2, 300, [0, 2, 3], ("0based", "half_open"))
A_RAW = ora.Side(A.chrom, A.start, A.end)      # CLUSTER / MERGE / GROUP BY read raw coordinates


def test_the_tables_are_the_shape_the_combiners_can_go_wrong_on():
    assert set(A.chrom) == {0, 1, 3} and set(B.chrom) == {0, 2, 3}
    keys = np.stack([A.chrom, A.start, A.end], 1)
    uniq, counts = np.unique(keys, axis=0, return_counts=True)
    assert {int(c) for c in uniq[counts > 1][:, 0]} == {0, 1, 3}                       # within every group
    assert np.unique(keys[:, 1:], axis=0).shape[0] < uniq.shape[0]                       # and across them
    assert max(A.cs.max(), A.ce.max(), B.cs.max(), B.ce.max()) < 100_000


def sub(side, rows):
    return ora.Side(side.chrom[rows], side.start[rows], side.end[rows], side.start_off, side.end_off)


def split(a, b=None):
    """``(rows_a, rows_b, sub_a, sub_b)`` per group, the row ids as ``HipEngine._groups`` yields them: ascending
    int64 tensors.  A one-table operator gets an empty B."""
    if b is None:
        b = ora.Side(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))
    for g in GROUPS:
        ra, rb = np.nonzero(np.isin(a.chrom, g))[0], np.nonzero(np.isin(b.chrom, g))[0]
        yield torch.from_numpy(ra), torch.from_numpy(rb), sub(a, ra), sub(b, rb)


def t(*arrays):
    """What an operator returns: one tensor, or a tuple of them."""
    out = tuple(torch.from_numpy(np.ascontiguousarray(x)) for x in arrays)
    return out[0] if len(out) == 1 else out


def parts_of(fn, a, b=None):
    return [(ra, rb, fn(sa, sb)) for ra, rb, sa, sb in split(a, b)]


def test_split_reaches_every_row_once_and_leaves_one_group_without_b():
    got = list(split(A, B))
    assert sorted(torch.cat([g[0] for g in got]).tolist()) == list(range(A.n))
    assert sorted(torch.cat([g[1] for g in got]).tolist()) == list(range(B.n))
    assert [g[3].n == 0 for g in got] == [False, True, False] and got[2][2].n == 0 and got[1][2].n > 30


def canon(s):
    return s.chrom, s.cs, s.ce


def as_i32(p):
    return p[:, 0].astype(np.int32), p[:, 1].astype(np.int32)


PAIR_ORACLES = {
    "inner": lambda a, b: ora.c_inner(a, b),
    "contain": lambda a, b: as_i32(C.contain_pairs(*canon(a), *canon(b))),
    "window": lambda a, b: as_i32(W.window_pairs(*canon(a), *canon(b), 250)),
}


@pytest.mark.parametrize("op", list(PAIR_ORACLES))
def test_pairs(op):
    fn = PAIR_ORACLES[op]
    ra, rb = wide.pairs(parts_of(lambda sa, sb: t(*fn(sa, sb)), A, B), CPU)
    want = ora.sort_pairs(*fn(A, B))
    assert ra.dtype == rb.dtype == torch.int32 and want.shape[0] > 100
    assert np.array_equal(ora.sort_pairs(ra.numpy(), rb.numpy()), want)


def test_pairs_come_in_group_order():
    parts = parts_of(lambda sa, sb: t(*ora.c_inner(sa, sb)), A, B)
    ra, rb = wide.pairs(parts, CPU)
    want_a = np.concatenate([rows[p[0].long()].numpy() for rows, _rb, p in parts])
    want_b = np.concatenate([rows[p[1].long()].numpy() for _ra, rows, p in parts])
    assert np.array_equal(ra.numpy(), want_a) and np.array_equal(rb.numpy(), want_b)


def test_per_row_count():
    got = wide.per_row(parts_of(lambda sa, sb: t(ora.c_count(sa, sb)), A, B), A.n, CPU)
    want = ora.c_count(A, B)
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want)
    assert want.sum() > 100 and not got.numpy()[A.chrom == 1].any()        # no B on chromosome 1: the zeros stay


@pytest.mark.parametrize("distance", [0, 300])
def test_per_row_cluster(distance):
    got = wide.per_row(parts_of(lambda s, _b: t(ora.c_cluster(s, distance)), A_RAW), A.n, CPU)
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), ora.c_cluster(A_RAW, distance))


def test_per_row_cluster_with_a_predicate():
    col = np.random.default_rng(3).integers(0, 2, A.n)

    def ids(s, col):
        return ora.py_cluster_predicate(s.chrom.tolist(), s.start.tolist(), s.end.tolist(), 300,
                                        lambda i, j: col[i] == col[j])

    # (the per-group call sees the predicate column's rows of that group: HipEngine._preds_of_rows)
    parts = [(ra, rb, t(ids(sa, col[ra.numpy()]))) for ra, rb, sa, _sb in split(A_RAW)]
    want = ids(A_RAW, col)
    assert np.array_equal(wide.per_row(parts, A.n, CPU).numpy(), want)
    assert not np.array_equal(want, ora.c_cluster(A_RAW, 300))             # the predicate decided somewhere


@pytest.mark.parametrize("signed, md", [(False, None), (True, 2000)])
@pytest.mark.parametrize("k", [1, 3])
def test_nearest(k, signed, md):
    if k == 1:
        fn, shape = (lambda a, b: ora.c_nearest_k1(a, b, signed=signed, max_distance=md)), (A.n,)
    else:
        fn, shape = (lambda a, b: ora.c_nearest_k(a, b, k, signed=signed, max_distance=md)), (A.n, k)
    idx, dist = wide.nearest(parts_of(lambda sa, sb: t(*fn(sa, sb)), A, B), shape, CPU)
    want_i, want_d = fn(A, B)
    assert idx.dtype == torch.int32 and dist.dtype == torch.int64 and tuple(idx.shape) == tuple(dist.shape) == shape
    assert np.array_equal(idx.numpy(), want_i) and np.array_equal(dist.numpy(), want_d)
    lone = A.chrom == 1                                                     # no B on chromosome 1
    assert (idx.numpy()[lone] == -1).all() and (dist.numpy()[lone] == 0).all() and (want_i[~lone] >= 0).any()
    if md is not None:
        assert (want_i[~lone] < 0).any()                                    # misses inside a group with a B
    if signed:
        assert (want_d < 0).any()


@pytest.mark.parametrize("anti", [False, True])
def test_row_ids(anti):
    got = wide.row_ids(parts_of(lambda sa, sb: t(ora.c_semi_anti(sa, sb, anti)), A, B), CPU)
    want = ora.c_semi_anti(A, B, anti)
    assert got.dtype == torch.int32 and want.size > 30 and np.array_equal(got.numpy(), want)


def np_group_rows(s):
    """Group ids ascending in (chrom, start, end) order and each group's first row, from one ``np.unique``."""
    keys = np.stack([s.chrom, s.start, s.end], 1).astype(np.int64)
    uniq, first, inv = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    return uniq, inv.reshape(-1).astype(np.int32), first.astype(np.int32)


def test_group_rows():
    parts = parts_of(lambda s, _b: t(*np_group_rows(s)[1:]), A_RAW)
    gid, rep = wide.group_rows(parts, *t(A.chrom, A.start, A.end))
    uniq, want_gid, want_rep = np_group_rows(A_RAW)
    assert gid.dtype == rep.dtype == torch.int32 and uniq.shape[0] < A.n
    assert np.array_equal(gid.numpy(), want_gid) and np.array_equal(rep.numpy(), want_rep)
    keys = np.stack([A.chrom, A.start, A.end], 1)
    assert np.array_equal(keys[rep.numpy()], uniq)


def np_disjoin(target, reference):
    """``brute_force_arrays`` sorts by (parent, start, end): the order the operator promises."""
    got = D.brute_force_arrays(*canon(target), *(canon(reference) if reference is not None else ()))
    return tuple(got[:, k].astype(np.int32) for k in range(3))


@pytest.mark.parametrize("mode", ["self", "reference"])
def test_disjoin(mode):
    ref = B if mode == "reference" else None
    parts = parts_of(lambda st, sr: t(*np_disjoin(st, sr if ref is not None else None)), A, ref)
    got = wide.disjoin(parts, CPU)
    want = np_disjoin(A, ref)
    assert all(x.dtype == torch.int32 for x in got) and want[0].size > 100
    # self mode cuts rows of two groups, which interleave in the whole table: concatenation alone leaves the parents
    # out of order (with a reference only the group that holds reference rows keeps pieces)
    assert ref is not None or (np.diff(np.concatenate([rows[p[0].long()].numpy() for rows, _rr, p in parts])) < 0).any()
    for g, w in zip(got, want):
        assert np.array_equal(g.numpy(), w)


@pytest.mark.parametrize("distance", [0, 300])
def test_merge(distance):
    parts = parts_of(lambda s, _b: t(*ora.c_merge(s, distance)), A_RAW)
    got = wide.merge(parts, CPU)
    want = ora.c_merge(A_RAW, distance)
    assert [x.dtype for x in got] == [torch.int32] * 3 + [torch.int64] and 10 < want[0].size < A.n
    for g, w in zip(got, want):
        assert np.array_equal(g.numpy(), w)
    # chromosome 3 shares a group with chromosome 0: concatenation alone would put it in front of chromosome 1
    assert not np.array_equal(torch.cat([p[0] for _rows, _rb, p in parts]).numpy(), want[0])


# ------------------------------------------------------------------ no group at all
def own_storage(*tensors):
    """No two of them share a storage (``data_ptr()`` of an empty tensor is 0 whatever it belongs to)."""
    return len({x.untyped_storage()._cdata for x in tensors}) == len(tensors)


def test_no_parts_pairs():
    ra, rb = wide.pairs([], CPU)
    assert ra.dtype == rb.dtype == torch.int32 and ra.shape == rb.shape == (0,)
    assert own_storage(ra, rb) and not ra.is_set_to(rb)


def test_no_parts_per_row_and_nearest():
    out = wide.per_row([], 5, CPU)
    assert out.dtype == torch.int64 and out.tolist() == [0] * 5
    for shape in ((4,), (4, 3)):
        idx, dist = wide.nearest([], shape, CPU)
        assert idx.dtype == torch.int32 and dist.dtype == torch.int64 and tuple(idx.shape) == tuple(dist.shape) == shape
        assert (idx == -1).all() and (dist == 0).all()


def test_no_parts_row_ids_group_rows_disjoin_merge():
    rows = wide.row_ids([], CPU)
    assert rows.dtype == torch.int32 and rows.shape == (0,)
    z = torch.empty(0, dtype=torch.int32)
    gid, rep = wide.group_rows([], z, z, z)
    assert gid.dtype == rep.dtype == torch.int32 and gid.shape == rep.shape == (0,) and own_storage(gid, rep)
    got = wide.disjoin([], CPU)
    assert len(got) == 3 and all(x.dtype == torch.int32 and x.shape == (0,) for x in got) and own_storage(*got)
    got = wide.merge([], CPU)
    assert [x.dtype for x in got] == [torch.int32] * 3 + [torch.int64] and all(x.shape == (0,) for x in got)
    assert own_storage(*got)
