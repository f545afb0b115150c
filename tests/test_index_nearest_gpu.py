"""NEAREST (k = 1, unstranded) against a table index (giql_hip_nearest_indexed_dev) -- needs a GPU.

The results are those of the ordinary operator (giql_hip_nearest_dev; the reference's lateral NEAREST,
src/giql/expanders/nearest.py:336-397 with the distance CASE of _distance.py:67-87), compared with the oracle's
``c_nearest_k1`` by the rule of test_gpu_parity.py::test_nearest_random_vs_oracle: the distances are equal, the same
rows have a target, the chosen target has the oracle's (start, end) -- and its row id where no other indexed row
shares that (chrom, start, end)."""

import numpy as np
import pytest

from giql_amd import synth
from oracle import pyoracle as ora
from test_gpu_parity import dev
from test_index_rows_gpu import ENCODINGS, boundary_tables, check_rows

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MODES = [(False, None), (True, None), (False, 500), (True, 2000)]      # (signed, max_distance)


@pytest.fixture(scope="module")
def eng():
    from giql_amd.engine import HipEngine

    e = HipEngine(0)
    yield e
    e.close()


def table(n, seed, kind, chroms=None):
    c, s, e = synth.make_table(n, seed, kind, chroms=chroms)
    return ora.Side(c, s, e)


def unique_rows(b):
    """Per row of ``b``: no other row shares its (chrom, start, end)."""
    rows = np.stack([b.chrom.astype(np.int64), b.cs, b.ce], 1)
    _, inverse, counts = np.unique(rows, axis=0, return_inverse=True, return_counts=True)
    return counts[inverse.reshape(-1)] == 1


def same_as_oracle(got, a, b, signed, md, what="", single=None):
    """The comparison rule of this file; returns the oracle's ``(idx, dist)``."""
    idx, dist = got
    assert idx.dtype == torch.int32 and dist.dtype == torch.int64, what
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    oi, od = ora.c_nearest_k1(a, b, signed=signed, max_distance=md, method="sweep")
    assert idx.shape == oi.shape and dist.shape == od.shape, what
    assert np.array_equal(dist, od), (what, np.nonzero(dist != od)[0][:5])
    assert np.array_equal(idx >= 0, oi >= 0), what
    m = oi >= 0
    assert idx[m].max(initial=0) < b.n, what
    assert np.array_equal(b.start[idx[m]], b.start[oi[m]]) and np.array_equal(b.end[idx[m]], b.end[oi[m]]), what
    assert np.array_equal(b.chrom[idx[m]], a.chrom[m]), what
    single = unique_rows(b) if single is None else single
    exact = m.copy()
    exact[m] = single[oi[m]]
    assert np.array_equal(idx[exact], oi[exact]), what
    return oi, od


def check_nearest(e, a, b, index, what="", modes=MODES, single=None):
    out = None
    for signed, md in modes:
        got = e.nearest_indexed(dev(a), index, signed=signed, max_distance=md)
        res = same_as_oracle(got, a, b, signed, md, (what, signed, md), single)
        out = out or res
        st = e.stats()
        assert st["n_a"] == a.n and st["n_b"] == b.n and st["n_out"] == a.n, st
    return out


@pytest.mark.parametrize("kind_b,general", [("reads", False), ("peaks", True)])
def test_both_forms_on_random_tables(eng, kind_b, general):
    b = table(300_000, 11, kind_b)
    single = unique_rows(b)
    index = eng.index_create(dev(b), 24)
    try:
        assert index.general == general
        created = index.nbytes
        index.prepare_nearest()
        grew = index.nbytes - created
        if general:
            assert grew >= 8 * b.n, grew          # row ids + prefix max in (start, end) order, the directory
        else:
            assert 0 < grew < 4 * b.n, grew       # the directory and a rank per chromosome
        index.prepare_nearest()                   # a second preparation changes nothing
        assert index.nbytes == created + grew
        for seed, n_a, kind_a in ((21, 50_000, "peaks"), (22, 20_000, "reads"), (23, 1_000, "peaks")):
            a = table(n_a, seed, kind_a)
            for _ in range(2):
                oi, od = check_nearest(eng, a, b, index, (seed, kind_a), single=single)
                assert (od == 0).any() and (od > 0).any() and (oi >= 0).all()
        assert index.nbytes == created + grew
        # the row operators prepare the same index afterwards (they find the directory there) ...
        a = table(20_000, 24, "peaks")
        before_rows = index.nbytes
        index.prepare_rows()
        if general:
            assert index.nbytes - before_rows >= 4 * b.n
        else:
            assert index.nbytes == before_rows    # all a fixed-length table needs is the directory NEAREST built
        want = check_rows(eng, a, b, index, "COUNT after NEAREST")
        assert (want == 0).any() and (want > 0).any()
        check_nearest(eng, a, b, index, "NEAREST after COUNT", single=single)
        # ... and the INNER join reads the index's own arrays, which NEAREST did not disturb
        ra, rb = eng.inner_join_indexed(dev(a), index)
        wa, wb = ora.c_inner(a, b, "sweep")
        assert np.array_equal(ora.sort_pairs(ra.cpu().numpy(), rb.cpu().numpy()), ora.sort_pairs(wa, wb))
    finally:
        index.close()


def test_prepare_rows_before_prepare_nearest(eng):
    b = table(300_000, 12, "peaks")
    index = eng.index_create(dev(b), 24)
    try:
        index.prepare_rows()
        after_rows = index.nbytes
        a = table(5_000, 25, "reads")
        check_nearest(eng, a, b, index, "first NEAREST call prepares")       # no prepare_nearest(): the call does it
        grew = index.nbytes - after_rows
        assert 8 * b.n <= grew < 8 * b.n + 4096, grew                          # the directory was found there
        want = check_rows(eng, a, b, index)
        assert (want > 0).any()
        assert index.nbytes == after_rows + grew
    finally:
        index.close()


@pytest.mark.parametrize("fixed_length", [False, True])
@pytest.mark.parametrize("enc_b", ENCODINGS)
def test_axis_edges_and_encodings(eng, enc_b, fixed_length):
    """The scenario of test_index_rows_gpu.py::test_axis_edges_and_encodings (query rows on chromosomes the index does
    not hold, beyond the indexed range, reaching over its end, starting below 0; every encoding pair) plus zero-length
    query rows inside a target, on its start and on its end."""
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
    # zero-length rows: inside a target, on its start, on its end (300 each, targets drawn from the indexed table)
    t = r.integers(0, n_b, 900)
    z = np.arange(150, 1050)
    ca[z] = cb[t]
    sa[z] = np.concatenate([sb[t[:300]] + lb[t[:300]] // 2, sb[t[300:600]], sb[t[600:]] + lb[t[600:]]])
    la[z] = 0
    b = ora.Side(cb, (sb - enc_b[0]).astype(np.int32), (sb + lb - enc_b[1]).astype(np.int32), enc_b[0], enc_b[1])
    single = unique_rows(b)
    last_end = np.array([int((sb + lb)[cb == c].max()) if (cb == c).any() else 0 for c in range(5)])
    index = eng.index_create(dev(b), 5)
    try:
        assert index.general == (not fixed_length)
        for ea in ENCODINGS:
            a = ora.Side(ca, (sa - ea[0]).astype(np.int32), (sa + la - ea[1]).astype(np.int32), ea[0], ea[1])
            oi, od = check_nearest(eng, a, b, index, (ea, enc_b), single=single)
            got_i, got_d = (x.cpu().numpy() for x in eng.nearest_indexed(dev(a), index))
            none = (ca >= 5) | (ca == 3)
            assert (got_i[none] == -1).all() and (got_d[none] == 0).all() and (got_i[~none] >= 0).all()
            beyond = ~none & (sa >= 30_000_400)       # past every indexed row: the true distance to the last target
            assert beyond.sum() > 500 and np.array_equal(got_d[beyond], sa[beyond] - last_end[ca[beyond]] + 1)
            assert int(got_d[beyond].max()) > 3_900_000
            inside, on_start, on_end = got_d[150:450], got_d[450:750], got_d[750:1050]
            assert (inside[lb[t[:300]] >= 2] == 0).all() and (on_start <= 1).all() and (on_end <= 1).all()
            assert (on_start == 1).any() and (on_end == 1).any()
    finally:
        index.close()


def general_boundary_table():
    """One chromosome, rows of variable length placed by hand around multiples of 2^13, 2^15 and 2^16 as start keys and
    as end keys, runs of 20 rows on one start with distinct, shuffled ends, buckets 4..6 of 2^16 keys left EMPTY
    between occupied ones; no two rows share (start, end)."""
    r = np.random.default_rng(78)
    bounds = [1 << 16, 2 << 16, 3 << 13, 5 << 15, 8 << 16, 9 << 16]
    s, ln = [], []
    for B in bounds:
        for d in (-1, 0, 1):
            s.append(B + d), ln.append(37)            # start keys on the places
            s.append(B + d - 61), ln.append(61)       # end keys on the places
        for start in (B, B - 200):                    # an equal-start run on the boundary and one ending around it
            s += [start] * 20
            ln += list(r.permutation(np.arange(190, 210)))
    fill = np.concatenate([r.integers(0, 262_144 - 600, 3_000), r.integers(524_288, 640_000, 1_500)])
    s += list(fill)
    ln += list(r.integers(1, 500, fill.size))
    rows = np.unique(np.stack([np.array(s, np.int64), np.array(s, np.int64) + np.array(ln, np.int64)], 1), axis=0)
    rows = rows[r.permutation(rows.shape[0])]
    return ora.Side(np.zeros(rows.shape[0], np.int32), rows[:, 0].astype(np.int32), rows[:, 1].astype(np.int32))


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
        a, b = boundary_tables(True)                  # the queries straddle, touch and just miss the boundaries
        if not fixed_length:
            b = general_boundary_table()
        extra_s = [300_000, 300_000, 400_000, 262_200, 0]      # inside the empty buckets; the whole chromosome
        extra_e = [300_100, 300_000, 400_001, 524_000, 700_000]
        a = ora.Side(np.zeros(a.n + 5, np.int32), np.concatenate([a.start, np.array(extra_s, np.int32)]),
                     np.concatenate([a.end, np.array(extra_e, np.int32)]))
        index = e.index_create(dev(b), 1)
        try:
            assert index.general == (not fixed_length)
            oi, od = check_nearest(e, a, b, index, bits)
            assert (od == 0).any() and (od > 0).any()
            far = (a.start == 300_000) | (a.start == 400_000)  # the nearest target lies several buckets away
            assert far.sum() >= 4 and (od[far] > 30_000).all() and (oi[far] >= 0).all()
            assert od[-1] == 0 and od[-2] > 0
            # the ordinary operator on the same context afterwards gives the same arrays
            gi, gd = (x.cpu().numpy() for x in e.nearest_indexed(dev(a), index, signed=True))
            wi, wd = (x.cpu().numpy() for x in e.nearest(dev(a), dev(b), 1, signed=True))
            assert np.array_equal(gd, wd) and np.array_equal(gi >= 0, wi >= 0)
            assert np.array_equal(b.start[gi], b.start[wi]) and np.array_equal(b.end[gi], b.end[wi])
            if not fixed_length:                      # no two rows share (start, end): the row ids agree too
                assert np.array_equal(gi, wi)
        finally:
            index.close()
    finally:
        e.close()


def test_ties_by_hand(eng):
    b = ora.make_side([
        (0, 100, 180), (0, 100, 130), (0, 100, 150), (0, 100, 120),      # 0-3: one start, scrambled ends
        (0, 300, 400), (0, 250, 400), (0, 350, 400),                     # 4-6: upstream rows sharing the largest end
        (0, 1000, 1010),                                                 # 7: the downstream row
        (0, 5000, 5003), (0, 5000, 5001), (0, 5000, 5002),               # 8-10
    ])
    a = ora.make_side([
        (0, 140, 160),      # overlaps 0 and 2: the smallest end that still exceeds a.start -> 2
        (0, 450, 460),      # upstream end 400 (d 51) beats 1000 (d 541): the smallest start -> 5
        (0, 600, 800),      # upstream 201 = downstream 201: upstream wins -> 5, negative when signed
        (0, 400, 420),      # book-ended upstream -> 5, distance 1
        (0, 990, 1000),     # book-ended downstream -> 7, distance 1
        (0, 601, 800),      # downstream nearer by one -> 7
        (0, 5001, 5001),    # zero length, overlapped by 10 and 8: (5000, 5002) first -> 10
        (0, 50, 60),        # before every row: downstream, the smallest end of the run -> 3
    ])
    index = eng.index_create(dev(b), 1)
    try:
        assert index.general
        for signed in (False, True):
            gi, gd = (x.cpu().numpy() for x in eng.nearest_indexed(dev(a), index, signed=signed))
            assert gi.tolist() == [2, 5, 5, 5, 7, 7, 10, 3], gi
            up = -1 if signed else 1
            assert gd.tolist() == [0, 51 * up, 201 * up, 1 * up, 1, 201, 0, 41], gd
            same_as_oracle(eng.nearest_indexed(dev(a), index, signed=signed), a, b, signed, None)
        gi, gd = (x.cpu().numpy() for x in eng.nearest_indexed(dev(a), index, max_distance=0))   # only the overlaps
        assert gi.tolist() == [2, -1, -1, -1, -1, -1, 10, -1] and not gd.any()
        same_as_oracle(eng.nearest_indexed(dev(a), index, signed=True, max_distance=1), a, b, True, 1)
    finally:
        index.close()


def test_declines_leave_everything_usable(eng):
    from giql_amd import _lib
    from giql_amd.engine import HipEngine

    b = table(300_000, 41, "reads")
    index = eng.index_create(dev(b), 24)
    try:
        q = table(20_000, 42, "peaks")
        q.end[3] = q.start[3] - 1                      # an inverted query row
        with pytest.raises(_lib.GiqlHipError) as ei:
            eng.nearest_indexed(dev(q), index)
        assert ei.value.code == _lib.GIQL_ERR_INVALID
        q.end[3] = q.start[3]                          # zero length: legal
        check_nearest(eng, q, b, index, "after an inverted row")
        empty = ora.Side(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))
        gi, gd = eng.nearest_indexed(dev(empty), index)
        assert gi.shape[0] == 0 and gd.shape[0] == 0 and gi.dtype == torch.int32 and gd.dtype == torch.int64
        other = HipEngine(0)
        try:
            with pytest.raises(ValueError):
                other.nearest_indexed(dev(q), index)
        finally:
            other.close()
    finally:
        index.close()
    # a general table with 3,000 rows on one start: the index does not take the NEAREST form, and remembers it
    r = np.random.default_rng(9)
    base = table(50_000, 43, "peaks")
    pile_s = np.full(3_000, 1_000_000, np.int32)
    pile = ora.Side(np.concatenate([base.chrom, np.full(3_000, 2, np.int32)]), np.concatenate([base.start, pile_s]),
                    np.concatenate([base.end, pile_s + r.integers(1, 5_000, 3_000).astype(np.int32)]))
    index = eng.index_create(dev(pile), 24)
    try:
        assert index.general
        q = table(5_000, 44, "peaks")
        before = index.nbytes
        for attempt in range(2):
            with pytest.raises(_lib.GiqlHipError) as ei:
                index.prepare_nearest()
            assert ei.value.code == _lib.GIQL_ERR_STATE and "ordinary operator" in str(ei.value), attempt
            with pytest.raises(_lib.GiqlHipError) as ei:
                eng.nearest_indexed(dev(q), index)
            assert ei.value.code == _lib.GIQL_ERR_STATE and "ordinary operator" in str(ei.value), attempt
            index._refresh_info()
            assert index.nbytes == before, attempt     # nothing of the attempt is kept
        want = check_rows(eng, q, pile, index, "COUNT on an index that declined NEAREST")
        assert (want > 0).any()
        same_as_oracle(eng.nearest(dev(q), dev(pile), 24), q, pile, False, None, "the ordinary operator")
    finally:
        index.close()


NEAREST_Q = ("SELECT a.chrom, a.start, a.score, b.start AS gs, b.\"end\" AS ge, b.score AS gscore, b.distance AS d "
             "FROM peaks a CROSS JOIN LATERAL NEAREST(genes, reference := a.interval, {args}) b")


def test_execute_answers_nearest_from_a_pinned_target_table(monkeypatch):
    pa = pytest.importorskip("pyarrow")
    import giql_amd
    from giql_amd import execute as ex
    from giql_amd.engine import DeviceSide, HipEngine
    from giql_amd.execute import execute
    from giql_amd.transpile import transpile

    names = np.array([f"chr{i + 1}" for i in range(24)])

    def arrow(side, unknown=False):
        chrom = names[side.chrom].astype(object)
        if unknown:
            chrom[:50], chrom[50:100] = "chrUn_1", "chrUn_2"   # two chromosomes the pinned table lacks
        # (the score is a function of the interval: rows sharing (chrom, start, end) are interchangeable targets)
        return pa.table({"chrom": pa.array(chrom, pa.string()), "start": pa.array(side.start), "end": pa.array(side.end),
                         "score": pa.array((side.start.astype(np.int64) + side.end) % 13),
                         "strand": pa.array(np.where(side.start % 2 == 0, "+", "-").astype(object), pa.string())})

    calls = {"index_create": 0, "nearest_indexed": 0, "nearest": 0, "nearest_k": 0}
    for name in calls:
        real = getattr(HipEngine, name)

        def wrapper(self, *a, _real=real, _name=name, **k):
            calls[_name] += 1
            return _real(self, *a, **k)

        monkeypatch.setattr(HipEngine, name, wrapper)
    uploads = []
    real_from_numpy = DeviceSide.from_numpy.__func__

    def from_numpy(cls, chrom, *a, **k):
        uploads.append(len(chrom))
        return real_from_numpy(cls, chrom, *a, **k)

    monkeypatch.setattr(DeviceSide, "from_numpy", classmethod(from_numpy))

    def same(got, want):
        key = [(c, "ascending") for c in want.column_names]
        return got.schema.equals(want.schema) and got.sort_by(key).equals(want.sort_by(key))

    def plan_of(args):
        return transpile(NEAREST_Q.format(args=args), tables=["peaks", "genes"], dialect="hip")

    routed = [plan_of("k := 1"), plan_of("k := 1, signed := true"), plan_of("k := 1, max_distance := 5000"),
              plan_of("k := 1, signed := true, max_distance := 20000")]
    monkeypatch.setitem(ex._INDEXED_NEAREST_FORMS, "general", True)
    monkeypatch.setitem(ex._INDEXED_NEAREST_FORMS, "fixed_length", True)
    genes = arrow(table(300_000, 51, "peaks"))
    right_uploads = []
    with giql_amd.pin(genes, index=True) as pinned:
        for seed, unknown in ((61, False), (62, True), (63, False)):
            peaks = arrow(table(20_000, seed, "peaks"), unknown)
            for plan in routed:
                before = dict(calls)
                del uploads[:]
                got = execute(plan, {"peaks": peaks, "genes": pinned})
                right_uploads.append(uploads.count(genes.num_rows))
                assert calls["nearest_indexed"] - before["nearest_indexed"] == 1, plan
                assert calls["nearest"] == before["nearest"] and calls["nearest_k"] == before["nearest_k"], plan
                want = execute(plan, {"peaks": peaks, "genes": genes})
                assert want.num_rows > 100 and same(got, want), (plan, seed, got.num_rows, want.num_rows)
                if unknown:
                    assert not any(c.startswith("chrUn") for c in got.column("chrom").to_pylist())
                    if '"max_distance":null' in plan:       # (a plan is its string form here)
                        assert got.num_rows == peaks.num_rows - 100
        # the target's columns went to the device once, for the index build, and never again
        assert right_uploads == [1] + [0] * 11, right_uploads
        # an INNER query on the same pin shares the index
        inner = transpile("SELECT a.start, a.score, b.start AS bs FROM peaks a JOIN genes b ON a.interval INTERSECTS b.interval",
                          tables=["peaks", "genes"], dialect="hip")
        assert same(execute(inner, {"peaks": peaks, "genes": pinned}), execute(inner, {"peaks": peaks, "genes": genes}))
        assert calls["index_create"] == 1 and len(pinned.index_info()) == 1
        # k > 1 and stranded: the ordinary operator, equal results
        before = dict(calls)
        for args in ("k := 2", "k := 1, stranded := true"):
            plan = plan_of(args)
            assert same(execute(plan, {"peaks": peaks, "genes": pinned}), execute(plan, {"peaks": peaks, "genes": genes}))
        assert calls["nearest_indexed"] == before["nearest_indexed"]
        assert calls["nearest"] + calls["nearest_k"] > before["nearest"] + before["nearest_k"]
        # the switch of the index's form turned off: the ordinary path
        monkeypatch.setitem(ex._INDEXED_NEAREST_FORMS, "general", False)
        before = dict(calls)
        assert same(execute(routed[0], {"peaks": peaks, "genes": pinned}), execute(routed[0], {"peaks": peaks, "genes": genes}))
        assert calls["nearest_indexed"] == before["nearest_indexed"] and calls["nearest"] == before["nearest"] + 2
        monkeypatch.setitem(ex._INDEXED_NEAREST_FORMS, "general", True)
    # only the LEFT table pinned: of no use to NEAREST
    with giql_amd.pin(peaks, index=True) as left:
        before = dict(calls)
        assert same(execute(routed[0], {"peaks": left, "genes": genes}), execute(routed[0], {"peaks": peaks, "genes": genes}))
        assert calls["nearest_indexed"] == before["nearest_indexed"] and calls["nearest"] == before["nearest"] + 2
        assert calls["index_create"] == 1 and left.index_info() == []
