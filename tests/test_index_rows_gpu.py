"""COUNT / SEMI / ANTI against a table index (giql_hip_count_indexed_dev / giql_hip_semi_anti_indexed_dev) -- needs a
GPU.

The results are those of the ordinary operators (bedtools -c / -u / -v; the reference's count_overlaps plan,
src/giql/expanders/intersects_duckdb.py:806-854): exact against the oracle's ``c_count`` / ``c_semi_anti``."""

import numpy as np
import pytest

from giql_amd import synth
from oracle import pyoracle as ora
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def eng():
    from giql_amd.engine import HipEngine

    e = HipEngine(0)
    yield e
    e.close()


def table(n, seed, kind, chroms=None):
    c, s, e = synth.make_table(n, seed, kind, chroms=chroms)
    return ora.Side(c, s, e)


def check_rows(e, a, b, index, what=""):
    """counts, SEMI rows and ANTI rows of ``a`` over ``index`` (built from ``b``) against the oracle; returns the
    oracle's counts."""
    want = ora.c_count(a, b)
    got = e.count_overlaps_indexed(dev(a), index)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want), what
    for anti in (False, True):
        rows = e.semi_anti_indexed(dev(a), index, anti)
        assert rows.dtype == torch.int32, what
        assert np.array_equal(rows.cpu().numpy(), np.sort(ora.c_semi_anti(a, b, anti))), (what, anti)
        assert np.array_equal(rows.cpu().numpy(), np.nonzero((want > 0) != anti)[0]), (what, anti)
    st = e.stats()
    assert st["n_a"] == a.n and st["n_b"] == b.n, st
    return want


def nontrivial(counts):
    return bool((counts == 0).any()) and bool((counts > 0).any())


@pytest.mark.parametrize("kind_b,general", [("reads", False), ("peaks", True)])
def test_one_index_serves_counts_semi_and_anti_in_both_forms(eng, kind_b, general):
    b = table(300_000, 11, kind_b)
    index = eng.index_create(dev(b), 24)
    try:
        assert index.general == general
        bytes_created = index.nbytes
        for seed, n_a, kind_a in ((21, 50_000, "peaks"), (22, 20_000, "reads"), (23, 1_000, "peaks")):
            a = table(n_a, seed, kind_a)
            for _ in range(2):
                assert nontrivial(check_rows(eng, a, b, index, (seed, kind_a)))
        grew = index.nbytes - bytes_created
        if general:
            assert grew >= 4 * b.n, grew          # the sorted end keys + two directories
        else:
            assert 0 < grew < 4 * b.n, grew       # one directory
        index.prepare_rows()                      # a second preparation changes nothing
        assert index.nbytes == bytes_created + grew
        a = table(20_000, 24, "peaks")
        assert nontrivial(check_rows(eng, a, b, index, "after a second prepare_rows"))
        # the INNER join reads the same index afterwards
        ra, rb = eng.inner_join_indexed(dev(a), index)
        wa, wb = ora.c_inner(a, b, "sweep")
        assert np.array_equal(ora.sort_pairs(ra.cpu().numpy(), rb.cpu().numpy()), ora.sort_pairs(wa, wb))
    finally:
        index.close()


def test_prepare_rows_before_the_first_call(eng):
    b = table(300_000, 12, "peaks")
    index = eng.index_create(dev(b), 24)
    try:
        before = index.nbytes
        index.prepare_rows()
        after = index.nbytes
        assert after - before >= 4 * b.n
        a = table(5_000, 25, "reads")
        assert nontrivial(check_rows(eng, a, b, index))
        assert index.nbytes == after
    finally:
        index.close()


ENCODINGS = [(0, 0), (0, 1), (-1, -1), (-1, 0)]     # (start_off, end_off) of engine.ENCODING_OFFSETS


@pytest.mark.parametrize("fixed_length", [False, True])
@pytest.mark.parametrize("enc_b", ENCODINGS)
def test_axis_edges_and_encodings(eng, enc_b, fixed_length):
    """The scenario of test_index_axis_edges_and_encodings: query rows on chromosomes the index does not hold (beyond
    its dictionary, and one inside it that no indexed row uses), beyond the indexed range, reaching over its end,
    starting below 0; every encoding pair (one indexed encoding per case, every query encoding against it)."""
    from giql_amd.engine import ENCODING_OFFSETS

    assert sorted(ENCODING_OFFSETS.values()) == sorted(ENCODINGS)
    encodings, enc_bs = ENCODINGS, [enc_b]
    r = np.random.default_rng(5)
    n_b = 100_000
    cb = r.integers(0, 5, n_b).astype(np.int32)
    cb[cb == 3] = 4                                   # chromosome 3: in no indexed row
    sb = r.integers(0, 30_000_000, n_b).astype(np.int64)
    lb = np.full(n_b, 150, np.int64) if fixed_length else r.integers(1, 400, n_b).astype(np.int64)
    n_a = 20_000
    ca = r.integers(0, 7, n_a).astype(np.int32)       # 5, 6: beyond the index's dictionary
    sa = r.integers(0, 34_000_000, n_a).astype(np.int64)   # some start beyond every indexed row
    la = r.integers(1, 3000, n_a).astype(np.int64)
    sa[:50] = 0
    sa[50:100] = 29_999_990                           # ... and some reach over the end of the indexed range
    sa[100:150] = -5                                  # below 0: some end at or below 0, some reach in
    la[100:125] = r.integers(1, 6, 25)
    for eb in enc_bs:
        b = ora.Side(cb, (sb - eb[0]).astype(np.int32), (sb + lb - eb[1]).astype(np.int32), eb[0], eb[1])
        index = eng.index_create(dev(b), 5)
        try:
            assert index.general == (not fixed_length)
            for ea in encodings:
                a = ora.Side(ca, (sa - ea[0]).astype(np.int32), (sa + la - ea[1]).astype(np.int32), ea[0], ea[1])
                want = check_rows(eng, a, b, index, (ea, eb))
                assert nontrivial(want) and not want[ca >= 5].any() and not want[ca == 3].any()
        finally:
            index.close()


def boundary_tables(fixed_length):
    """One chromosome; index rows and query rows placed by hand around multiples of 2^13, 2^15 and 2^16 (the
    bucket widths the test runs with: chromosome 0 starts at key 0, so positions are keys)."""
    r = np.random.default_rng(77)
    L = 100
    bounds = [1 << 16, 2 << 16, 3 << 13, 5 << 15, 8 << 16, 9 << 16]
    s, ln = [], []
    for B in bounds:
        for d in (-1, 0, 1):                          # start keys (k << w) - 1, k << w, (k << w) + 1
            s.append(B + d), ln.append(37)
        for d in (-1, 0, 1):                          # end keys on the same places
            s.append(B + d - 61), ln.append(61)
    s += [200_000] * 3_000                            # a few thousand rows sharing one start
    ln += list(r.integers(1, 500, 3_000))
    # buckets 4..6 of 2^16 keys, [262144, 458752), stay EMPTY between occupied ones (bucket 7 holds only the
    # hand-placed rows just below 8 << 16)
    fill = np.concatenate([r.integers(0, 262_144 - 600, 3_000), r.integers(524_288, 640_000, 1_500)])
    s += list(fill)
    ln += list(r.integers(1, 500, fill.size))
    s, ln = np.array(s, np.int64), np.array(ln, np.int64)
    if fixed_length:
        ln[:] = L
        # (end keys on the boundaries again, for this length)
        extra = np.array([B + d - L for B in bounds for d in (-1, 0, 1)], np.int64)
        s, ln = np.concatenate([s, extra]), np.concatenate([ln, np.full(extra.size, L)])
    p = r.permutation(s.size)
    b = ora.Side(np.zeros(s.size, np.int32), s[p].astype(np.int32), (s + ln)[p].astype(np.int32))
    qs, qe = [], []
    for B in bounds + [200_000]:
        for lo, hi in ((B, B + 10), (B - 10, B), (B - 1, B), (B, B + 1), (B + 1, B + 2), (B - 40, B + 40),
                       (B - 101, B - 100), (B + 36, B + 37), (B + 37, B + 38)):
            qs.append(lo), qe.append(hi)
    qs += [0, 300_000, 300_000, 262_144, 524_287, 639_999, 700_000]     # the whole chromosome; inside the empty buckets
    qe += [700_000, 300_100, 300_001, 524_288, 524_288, 640_600, 700_010]
    rs = r.integers(0, 650_000, 3_000)
    qs += list(rs)
    qe += list(rs + r.integers(1, 2_000, 3_000))
    p = r.permutation(len(qs))
    a = ora.Side(np.zeros(len(qs), np.int32), np.array(qs, np.int32)[p], np.array(qe, np.int32)[p])
    return a, b


@pytest.mark.parametrize("fixed_length", [False, True])
@pytest.mark.parametrize("bits", [0, 13, 15])
def test_bucket_boundaries(monkeypatch, bits, fixed_length):
    from giql_amd.engine import HipEngine

    if bits:
        monkeypatch.setenv("GIQL_HIP_LOCAL_BITS", str(bits))
    e = HipEngine(0)
    if bits:
        monkeypatch.delenv("GIQL_HIP_LOCAL_BITS")
    try:
        a, b = boundary_tables(fixed_length)
        assert int((a.end.astype(np.int64) - a.start).max()) > 32_768      # accepted here: no window cap
        index = e.index_create(dev(b), 1)
        try:
            assert index.general == (not fixed_length)
            want = check_rows(e, a, b, index, bits)
            assert nontrivial(want) and int(want.max()) >= b.n - 10         # the whole-chromosome row
            assert want[(a.start == 300_000)].max() == 0                    # the empty buckets
            # the ordinary operator on the same context afterwards
            assert np.array_equal(e.count_overlaps(dev(a), dev(b), 1).cpu().numpy(), want)
        finally:
            index.close()
    finally:
        e.close()


def test_declines_leave_the_context_usable(eng):
    from giql_amd import _lib

    b = table(300_000, 41, "reads")
    index = eng.index_create(dev(b), 24)
    try:
        q = table(20_000, 42, "peaks")
        q.end[3] = q.start[3]                          # an irregular query row on an indexed chromosome
        with pytest.raises(_lib.GiqlHipError) as ei:
            eng.count_overlaps_indexed(dev(q), index)
        assert ei.value.code == _lib.GIQL_ERR_STATE and "ordinary operator" in str(ei.value)
        for anti in (False, True):
            with pytest.raises(_lib.GiqlHipError) as ei:
                eng.semi_anti_indexed(dev(q), index, anti)
            assert ei.value.code == _lib.GIQL_ERR_STATE
        q2 = table(20_000, 43, "peaks")
        want = check_rows(eng, q2, b, index)
        assert np.array_equal(eng.count_overlaps(dev(q2), dev(b), 24).cpu().numpy(), want)
        # ... the ordinary operator answers the irregular table
        assert np.array_equal(eng.count_overlaps(dev(q), dev(b), 24).cpu().numpy(), ora.c_count(q, b))
        empty = ora.Side(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))
        assert eng.count_overlaps_indexed(dev(empty), index).shape[0] == 0
        assert eng.semi_anti_indexed(dev(empty), index, False).shape[0] == 0
        assert eng.semi_anti_indexed(dev(empty), index, True).shape[0] == 0
        # an index of another engine is refused
        from giql_amd.engine import HipEngine

        other = HipEngine(0)
        try:
            with pytest.raises(ValueError):
                other.count_overlaps_indexed(dev(q2), index)
            with pytest.raises(ValueError):
                other.semi_anti_indexed(dev(q2), index, False)
        finally:
            other.close()
    finally:
        index.close()


COUNT_KEYS = ('SELECT a.chrom, a.start, a."end", COUNT(b.chrom) AS n FROM peaks a LEFT JOIN reads b '
              'ON a.interval INTERSECTS b.interval GROUP BY a.chrom, a.start, a."end"')
COUNT_OTHER = ('SELECT a.chrom, a.score, COUNT(b.chrom) AS n FROM peaks a LEFT JOIN reads b '
               'ON a.interval INTERSECTS b.interval GROUP BY a.chrom, a.score')
SEMI_Q = "SELECT a.chrom, a.start, a.score FROM peaks a SEMI JOIN reads b ON a.interval INTERSECTS b.interval"
ANTI_Q = "SELECT a.chrom, a.start, a.score FROM peaks a ANTI JOIN reads b ON a.interval INTERSECTS b.interval"


def test_execute_answers_row_plans_from_a_pinned_right_table(monkeypatch):
    pa = pytest.importorskip("pyarrow")
    import giql_amd
    from giql_amd.engine import HipEngine
    from giql_amd.execute import execute
    from giql_amd.transpile import transpile

    names = np.array([f"chr{i + 1}" for i in range(24)])

    def arrow(side, unknown=False):
        chrom = names[side.chrom].astype(object)
        start, end = side.start.copy(), side.end.copy()
        if unknown:
            # two chromosomes the pinned table lacks, holding rows with identical (start, end)
            chrom[:50], chrom[50:100] = "chrUn_1", "chrUn_2"
            start[50:100], end[50:100] = start[:50], end[:50]
        return pa.table({"chrom": pa.array(chrom, pa.string()), "start": pa.array(start), "end": pa.array(end),
                         "score": pa.array(np.arange(side.n, dtype=np.int32) % 13)})

    calls = {"index_create": 0, "count_overlaps_indexed": 0, "semi_anti_indexed": 0, "count_overlaps": 0, "semi_anti": 0}

    def counted(name):
        real = getattr(HipEngine, name)

        def wrapper(self, *a, **k):
            calls[name] += 1
            return real(self, *a, **k)

        monkeypatch.setattr(HipEngine, name, wrapper)

    for name in calls:
        counted(name)

    # uploads of a table of the pinned table's size: the index build is the only one the indexed path may make
    from giql_amd.engine import DeviceSide

    uploads = []
    real_from_numpy = DeviceSide.from_numpy.__func__

    def from_numpy(cls, chrom, *a, **k):
        uploads.append(len(chrom))
        return real_from_numpy(cls, chrom, *a, **k)

    monkeypatch.setattr(DeviceSide, "from_numpy", classmethod(from_numpy))
    right_uploads = []                                 # per indexed execute(): uploads of reads.n rows

    def same(got, want):
        key = [(c, "ascending") for c in want.column_names]
        return got.schema.equals(want.schema) and got.sort_by(key).equals(want.sort_by(key))

    plans = {q: transpile(q, tables=["peaks", "reads"], dialect="hip") for q in (COUNT_KEYS, COUNT_OTHER, SEMI_Q, ANTI_Q)}
    reads = arrow(table(300_000, 51, "reads"))
    with giql_amd.pin(reads, index=True) as pinned:
        for seed, unknown in ((61, False), (62, True), (63, False)):
            peaks = arrow(table(20_000, seed, "peaks"), unknown)
            for q, plan in plans.items():
                before = dict(calls)
                del uploads[:]
                got = execute(plan, {"peaks": peaks, "reads": pinned})
                right_uploads.append(uploads.count(reads.num_rows))
                ordinary = calls["count_overlaps"] + calls["semi_anti"] - before["count_overlaps"] - before["semi_anti"]
                indexed = (calls["count_overlaps_indexed"] + calls["semi_anti_indexed"]
                           - before["count_overlaps_indexed"] - before["semi_anti_indexed"])
                assert (ordinary, indexed) == (0, 1), (q, ordinary, indexed)
                want = execute(plan, {"peaks": peaks, "reads": reads})
                assert want.num_rows > 100 and same(got, want), (q, seed, got.num_rows, want.num_rows)
                if unknown and q == COUNT_KEYS:
                    # the GPU GROUP BY keeps the two unknown chromosomes apart
                    chroms = got.column("chrom").to_pylist()
                    assert chroms.count("chrUn_1") >= 40 and chroms.count("chrUn_2") >= 40
                    un1 = {(s, e) for c, s, e in zip(chroms, got.column("start").to_pylist(), got.column("end").to_pylist())
                           if c == "chrUn_1"}
                    un2 = {(s, e) for c, s, e in zip(chroms, got.column("start").to_pylist(), got.column("end").to_pylist())
                           if c == "chrUn_2"}
                    assert un1 == un2 and len(un1) >= 40
        # the right table's columns went to the device once, for the index build, and never again
        assert right_uploads == [1] + [0] * 11, right_uploads
        # an INNER query on the same pin shares the index
        inner = transpile("SELECT a.start, a.score, b.start AS bs FROM peaks a JOIN reads b ON a.interval INTERSECTS b.interval",
                          tables=["peaks", "reads"], dialect="hip")
        got = execute(inner, {"peaks": peaks, "reads": pinned})
        assert same(got, execute(inner, {"peaks": peaks, "reads": reads}))
        assert calls["index_create"] == 1 and len(pinned.index_info()) == 1
        # a residual: the ordinary path
        before = dict(calls)
        resid = transpile(SEMI_Q + " AND a.score > 2", tables=["peaks", "reads"], dialect="hip")
        got = execute(resid, {"peaks": peaks, "reads": pinned})
        assert calls["semi_anti_indexed"] == before["semi_anti_indexed"]
        assert same(got, execute(resid, {"peaks": peaks, "reads": reads}))
    # only the LEFT table pinned: of no use to the row operators
    with giql_amd.pin(peaks, index=True) as left:
        before = dict(calls)
        for q in (COUNT_KEYS, SEMI_Q, ANTI_Q):
            got = execute(plans[q], {"peaks": left, "reads": reads})
            assert same(got, execute(plans[q], {"peaks": peaks, "reads": reads}))
        assert calls["count_overlaps_indexed"] == before["count_overlaps_indexed"]
        assert calls["semi_anti_indexed"] == before["semi_anti_indexed"]
        assert calls["index_create"] == 1 and left.index_info() == []
