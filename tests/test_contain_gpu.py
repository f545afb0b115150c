"""Column-to-column CONTAINS / WITHIN joins on the GPU: the golden fixture through HipEngine.contain_join and through
transpile + execute, both forms of the plan, the edges of the general form's candidate tiles, the uniform form's
length edges, irregular rows, candidate indices past 2^32, the plan / fill protocol, keys at the top of the 32-bit
axis with the chromosome-group fallback, residuals beside the predicate, and the zero-length rows an INTERSECTS join
plus comparisons cannot find.  Integers throughout: every comparison is exact."""

import ctypes
import os
import re

import numpy as np
import pytest

import _contain_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pa = pytest.importorskip("pyarrow")

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ct_constant(name):
    text = open(os.path.join(ROOT, "giql_amd", "csrc", "contain_kernels.hip.h")).read()
    return int(re.search(rf"constexpr int {name} = (\d+);", text).group(1))


CT_TILE = _ct_constant("CT_NT") * _ct_constant("CT_ITEMS")     # candidates per block of the general form
CT_QCAP = _ct_constant("CT_QCAP")                              # outer rows a tile stages in LDS


def _new_engine(env=()):
    from giql_amd.engine import HipEngine

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    with pytest.MonkeyPatch.context() as mp:
        for k, v in env:
            mp.setenv(k, v)
        return HipEngine(0)


@pytest.fixture(scope="module")
def eng():
    e = _new_engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_local():
    """A context that sorts in three stages whatever the size (tests/test_sort_stages.py)."""
    e = _new_engine([("GIQL_HIP_LOCAL_MIN_ROWS", "1")])
    yield e
    e.close()


def _side(chrom, start, end, offsets=(0, 0)):
    from giql_amd.engine import DeviceSide

    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.int32)).to(DEV)
    return DeviceSide(t(chrom), t(start), t(end), offsets[0], offsets[1])


def _pairs(ro, ri):
    return R.sort_pairs(np.stack([ro.cpu().numpy(), ri.cpu().numpy()], 1))


def _contain(eng, outer, inner, n_chrom, form=None):
    """contain_join of two ``(chrom, start, end)`` canonical triples -> sorted pairs; asserts the form when given."""
    got = _pairs(*eng.contain_join(_side(*outer), _side(*inner), n_chrom))
    if form is not None:
        assert eng.stats()["join_form"] == form, eng.stats()
    assert eng.stats()["n_out"] == got.shape[0]
    return got


# ------------------------------------------------------------------ the fixture
CASES = R.golden_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_golden_engine(eng, case):
    ac, as_, ae, offs_a, bc, bs, be, offs_b, n_chrom = R.case_arrays(case)
    a, b = _side(ac, as_, ae, offs_a), _side(bc, bs, be, offs_b)
    contains = _pairs(*eng.contain_join(a, b, n_chrom))
    st = eng.stats()
    assert contains.tolist() == case["contains"]
    uniform = any(t.startswith("uniform-inner-L") for t in case["tags"])
    assert st["join_form"] == ("uniform_b" if uniform else "general") or len({r[2] - r[1] for r in case["b"]}) == 1, st
    assert st["n_irregular_a"] == sum(r[2] + offs_a[1] <= r[1] + offs_a[0] for r in case["a"])
    assert st["n_irregular_b"] == sum(r[2] + offs_b[1] <= r[1] + offs_b[0] for r in case["b"])
    # a WITHIN b = contain(b, a) with the columns exchanged; and it is the transpose of b CONTAINS a
    rb, ra = eng.contain_join(b, a, n_chrom)
    assert _pairs(ra, rb).tolist() == case["within"]
    assert _pairs(rb, ra).tolist() == R.case_brute_force({**case, "a": case["b"], "b": case["a"], "enc_a": case["enc_b"],
                                                         "enc_b": case["enc_a"]}, "contains")


def _table(rows, score_seed=None):
    cols = {"chrom": pa.array([r[0] for r in rows], pa.string()),
            "start": pa.array([r[1] for r in rows], pa.int32()),
            "end": pa.array([r[2] for r in rows], pa.int32()),
            "rid": pa.array(list(range(len(rows))), pa.int32())}
    if score_seed is not None:
        cols["score"] = pa.array(np.random.default_rng(score_seed).integers(0, 6, len(rows)).astype(np.int32))
    return pa.table(cols)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_golden_execute(eng, case):
    from giql_amd.execute import execute
    from giql_amd.table import Table
    from giql_amd.transpile import transpile

    tables = [Table("ta", coordinate_system=case["enc_a"][0], interval_type=case["enc_a"][1]),
              Table("tb", coordinate_system=case["enc_b"][0], interval_type=case["enc_b"][1])]
    data = {"ta": _table(case["a"]), "tb": _table(case["b"])}
    got = {}
    for word, query in (("contains", "SELECT a.rid AS ra, b.rid AS rb FROM ta a JOIN tb b ON a.interval CONTAINS b.interval"),
                        ("within", "SELECT a.rid AS ra, b.rid AS rb FROM ta a, tb b WHERE a.interval WITHIN b.interval"),
                        ("swapped", "SELECT a.rid AS ra, b.rid AS rb FROM tb b JOIN ta a ON b.interval WITHIN a.interval")):
        out = execute(transpile(query, tables, dialect="hip"), data, eng)
        got[word] = R.sort_pairs(np.stack([out.column("ra").to_numpy(), out.column("rb").to_numpy()], 1)).tolist()
    assert got["contains"] == case["contains"]
    assert got["within"] == case["within"]
    assert got["swapped"] == case["contains"]          # b WITHIN a: the transpose of a CONTAINS b, same tables


# ------------------------------------------------------------------ general form: candidate tiles
def _tile_case(n_first, n_zero_rows, n_second, seed, by_tile=False):
    """One chromosome.  Outer row A = [0, 10^6) owns ``n_first`` candidates (distinct starts), then ``n_zero_rows``
    outer rows that own none, then outer row B = [2*10^6, 3*10^6) with ``n_second``.  A's inner rows end at A's end or
    one past it at random; ``by_tile``: in start order the first CT_TILE of them end past A (a tile in which nothing
    passes) and the next CT_TILE inside it (a tile in which everything passes)."""
    r = np.random.default_rng(seed)
    big = 10**6
    s1 = np.sort(r.choice(big - 10, n_first, replace=False))
    pos = np.arange(n_first)
    mixed = np.where(r.random(n_first) < 0.5, np.minimum(s1 + 1 + r.integers(0, 9, n_first), big), big + 1)
    e1 = mixed
    if by_tile:
        e1 = np.where(pos < CT_TILE, big + 1 + r.integers(0, 50, n_first),
                      np.where(pos < 2 * CT_TILE, np.minimum(s1 + 1 + r.integers(0, 9, n_first), big), mixed))
    s2 = r.integers(2 * big, 3 * big - 10, n_second)
    e2 = np.where(r.random(n_second) < 0.5, s2 + 1 + r.integers(0, 9, n_second), 3 * big + 7)
    zs = big + 10 + 3 * np.arange(n_zero_rows)            # outer rows between A and B: no inner row starts there
    os_ = np.concatenate([[0], zs, [2 * big]])
    oe = np.concatenate([[big], zs + 2, [3 * big]])
    is_ = np.concatenate([s1, s2])
    ie = np.concatenate([e1, e2])
    po, pi = r.permutation(os_.size), r.permutation(is_.size)
    return ((np.zeros(os_.size, np.int64), os_[po], oe[po]), (np.zeros(is_.size, np.int64), is_[pi], ie[pi]),
            n_first + n_second)


@pytest.mark.parametrize("total", [CT_TILE - 1, CT_TILE, CT_TILE + 1, 2 * CT_TILE + 1], ids=lambda t: f"T{t}")
def test_candidate_total_at_the_tile_edges(eng, total):
    outer, inner, t = _tile_case(total, 0, 0, total)
    assert t == total and outer[0].size + inner[0].size < 50_000
    got = _contain(eng, outer, inner, 1, "general")
    want = R.contain_pairs(*outer, *inner)
    assert 0 < want.shape[0] < total and np.array_equal(got, want)


def test_one_row_over_three_tiles_with_an_empty_and_a_full_tile(eng):
    n = 3 * CT_TILE + 100
    outer, inner, _ = _tile_case(n, 0, 0, 7, by_tile=True)
    assert n + 2 < 50_000
    ends = inner[2][np.argsort(inner[1])]                # A's candidates in the order of the sorted inner side
    assert (ends[:CT_TILE] > 10**6).all() and (ends[CT_TILE: 2 * CT_TILE] <= 10**6).all()
    assert 0 < (ends[2 * CT_TILE:] <= 10**6).sum() < n - 2 * CT_TILE
    got = _contain(eng, outer, inner, 1, "general")
    assert np.array_equal(got, R.contain_pairs(*outer, *inner))


@pytest.mark.parametrize("n_zero", [3, CT_QCAP + 200], ids=["staged", "past-the-lds-stage"])
@pytest.mark.parametrize("n_first", [CT_TILE - 5, CT_TILE], ids=["inside", "at-the-boundary"])
def test_tiles_that_begin_with_rows_without_candidates(eng, n_first, n_zero):
    # the rows without candidates sit at candidate offset n_first: inside tile 0 (with B's first 5 candidates behind
    # them) or exactly at the start of tile 1; more of them than a tile stages sends tile 0 to the search in HBM
    outer, inner, t = _tile_case(n_first, n_zero, 300, n_first + n_zero)
    assert t == n_first + 300 and outer[0].size + inner[0].size < 50_000
    got = _contain(eng, outer, inner, 1, "general")
    want = R.contain_pairs(*outer, *inner)
    owners = np.unique(want[:, 0])
    assert owners.size == 2                              # only A and B own pairs
    assert np.array_equal(got, want)


# ------------------------------------------------------------------ uniform form
def test_uniform_inner_side_and_the_switch_to_the_general_form(eng):
    L = 5
    r = np.random.default_rng(11)
    n_o, n_i = 600, 3000
    os_ = r.integers(0, 4000, n_o)
    ln = np.concatenate([r.integers(1, L, 200), np.full(200, L), r.integers(L + 1, 60, 200)])   # shorter, equal, longer
    oc = r.integers(0, 2, n_o)
    is_ = r.integers(0, 4000, n_i)
    ic = r.integers(0, 2, n_i)
    is_[:200], ic[:200] = os_[200:400], oc[200:400]       # inner rows identical to the outer rows of length L
    outer, inner = (oc, os_, os_ + ln), (ic, is_, is_ + L)
    got = _contain(eng, outer, inner, 2, "uniform_b")
    want = R.contain_pairs(*outer, *inner)
    assert np.array_equal(got, want)
    per_outer = np.bincount(want[:, 0], minlength=n_o)
    assert per_outer[:200].sum() == 0 and (per_outer[200:400] >= 1).all() and per_outer[400:].sum() > 0
    # L = 1 (variants in genes)
    inner1 = (ic, is_, is_ + 1)
    assert np.array_equal(_contain(eng, outer, inner1, 2, "uniform_b"), R.contain_pairs(*outer, *inner1))
    # one inner row a position longer: the general form, and (the row is contained in nothing either way) the same answer
    lonely = int(np.argmax(~np.isin(np.arange(n_i), want[:, 1])))
    ie2 = is_ + L
    ie2[lonely] += 1
    inner2 = (ic, is_, ie2)
    want2 = R.contain_pairs(*outer, *inner2)
    assert np.array_equal(want2, want)
    assert np.array_equal(_contain(eng, outer, inner2, 2, "general"), want)


# ------------------------------------------------------------------ irregular rows
@pytest.mark.parametrize("where", ["outer", "inner", "both"])
def test_irregular_rows_on_either_side(eng, where):
    r = np.random.default_rng({"outer": 1, "inner": 2, "both": 3}[where])
    n = 800
    oc, os_ = r.integers(0, 3, n), r.integers(0, 3000, n)
    oe = os_ + r.integers(1, 400, n)
    ic, is_ = r.integers(0, 3, n), r.integers(0, 3000, n)
    ie = is_ + r.integers(1, 60, n)
    irr_o = np.zeros(n, bool)
    irr_i = np.zeros(n, bool)
    if where in ("outer", "both"):
        irr_o[:60] = True
        oe[:40] = os_[:40]                      # zero-length
        oe[40:60] = os_[40:60] - r.integers(1, 30, 20)   # inverted
        ic[:40], is_[:40], ie[:40] = oc[:40], os_[:40], os_[:40] + (0 if where == "both" else 1)
    if where in ("inner", "both"):
        lo = 100
        irr_i[lo:lo + 60] = True
        ie[lo:lo + 40] = is_[lo:lo + 40]
        ie[lo + 40:lo + 60] = is_[lo + 40:lo + 60] - r.integers(1, 30, 20)
    outer, inner = (oc, os_, oe), (ic, is_, ie)
    got = _contain(eng, outer, inner, 3, "general")
    st = eng.stats()
    assert (st["n_irregular_a"], st["n_irregular_b"]) == (int((oe <= os_).sum()), int((ie <= is_).sum()))
    want = R.contain_pairs(*outer, *inner)
    assert np.array_equal(got, want)
    part_x = (oe <= os_)[want[:, 0]]                               # irregular outer x any inner
    part_y = ~part_x & (ie <= is_)[want[:, 1]]                     # regular outer x irregular inner
    # an irregular outer row can hold only an irregular inner row (o.start <= i.start and i.end <= o.end <= o.start
    # give i.end <= i.start), so with regular inner rows part X runs over the near misses above and must add nothing
    assert (part_x.sum() > 0) == (where == "both") and (part_y.sum() > 0) == (where in ("inner", "both"))
    assert (~part_x & ~part_y).sum() > 1000                        # and the regular pairs are still exact


def test_zero_length_rows_an_intersects_join_cannot_find(eng):
    from giql_amd.execute import execute
    from giql_amd.transpile import transpile

    rows = [["chr1", 5, 5], ["chr1", 0, 10]]
    data = {"ta": _table(rows), "tb": _table(rows)}
    contains = execute(transpile("SELECT a.rid AS ra, b.rid AS rb FROM ta a JOIN tb b ON a.interval CONTAINS b.interval",
                                 ["ta", "tb"], dialect="hip"), data, eng)
    got = sorted(zip(contains.column("ra").to_pylist(), contains.column("rb").to_pylist()))
    assert got == [(0, 0), (1, 0), (1, 1)]               # [5,5) CONTAINS [5,5)
    via_overlap = execute(transpile("SELECT a.rid AS ra, b.rid AS rb FROM ta a JOIN tb b ON a.interval INTERSECTS b.interval "
                                    "AND a.start <= b.start AND a.end >= b.end", ["ta", "tb"], dialect="hip"), data, eng)
    missed = sorted(zip(via_overlap.column("ra").to_pylist(), via_overlap.column("rb").to_pylist()))
    assert missed == [(1, 0), (1, 1)]                    # the two zero-length rows do not intersect


# ------------------------------------------------------------------ 64-bit candidate indices
def test_candidate_indices_past_32_bits(eng):
    n = 70_000
    i = np.arange(n)
    outer = (np.zeros(n, np.int64), np.zeros(n, np.int64), np.full(n, 1000))
    passing = i % 1000 == 0
    inner = (np.zeros(n, np.int64), i % 500, np.where(passing, 1000, 1001 + i % 7))
    ro, ri = eng.contain_join(_side(*outer), _side(*inner), 1)
    st = eng.stats()
    assert st["join_form"] == "general" and n * n > 2**32          # T = 4.9e9 candidates
    assert ro.shape[0] == ri.shape[0] == st["n_out"] == 70 * n     # P = 4.9M pairs
    assert torch.equal(torch.bincount(ro.long(), minlength=n), torch.full((n,), 70, device=DEV))
    want_inner = torch.from_numpy(np.where(passing, n, 0)).to(DEV)
    assert torch.equal(torch.bincount(ri.long(), minlength=n), want_inner)


# ------------------------------------------------------------------ plan / fill protocol
def test_plan_fill_protocol(eng):
    from giql_amd import _lib

    L, h, st = eng._L, eng._h, eng._stream()
    r = np.random.default_rng(5)
    n = 500
    os_, is_ = r.integers(0, 2000, n), r.integers(0, 2000, n)
    outer = (np.zeros(n, np.int64), os_, os_ + r.integers(1, 300, n))
    inner = (np.zeros(n, np.int64), is_, is_ + r.integers(1, 40, n))
    want = R.contain_pairs(*outer, *inner)
    o, i = _side(*outer), _side(*inner)
    co, ci = o.c_struct(), i.c_struct()
    cnt = ctypes.c_int64(-1)

    def plan(a=co, b=ci):
        return L.giql_hip_contain_plan_dev(h, ctypes.byref(a), ctypes.byref(b), 1, st, ctypes.byref(cnt))

    def fill(cap=None):
        ro = torch.empty(want.shape[0], dtype=torch.int32, device=DEV)
        ri = torch.empty_like(ro)
        rc = L.giql_hip_contain_fill_dev(h, ro.data_ptr(), ri.data_ptr(), want.shape[0] if cap is None else cap, st)
        return rc, ro, ri

    # two plans in a row, a short capacity (the plan stays valid), then the fill
    assert plan() == 0 and plan() == 0 and cnt.value == want.shape[0] > 0
    assert fill(cap=want.shape[0] - 1)[0] == _lib.GIQL_ERR_CAPACITY
    rc, ro, ri = fill()
    assert rc == 0 and np.array_equal(_pairs(ro, ri), want)
    rc, ro, ri = fill()                                   # the plan is still there
    assert rc == 0 and np.array_equal(_pairs(ro, ri), want)
    assert L.giql_hip_contain_fill_dev(h, None, None, want.shape[0], st) == _lib.GIQL_ERR_INVALID
    # an INNER fill or a plan export after a contain plan
    assert L.giql_hip_inner_fill_dev(h, ro.data_ptr(), ri.data_ptr(), want.shape[0], st) == _lib.GIQL_ERR_STATE
    with pytest.raises(_lib.GiqlHipError) as ei:
        eng.plan_sizes()
    assert ei.value.code == _lib.GIQL_ERR_STATE
    assert fill()[0] == 0                                 # neither of them launched anything
    # a fill after another operator, and a contain fill after an INNER plan
    eng.count_overlaps(o, i, 1)
    assert fill()[0] == _lib.GIQL_ERR_STATE
    assert plan() == 0
    assert eng.inner_plan(o, i, 1) > 0
    assert fill()[0] == _lib.GIQL_ERR_STATE
    # empty sides: zero pairs, a valid (empty) plan, no launch
    empty = _side([], [], []).c_struct()
    for a, b in ((empty, ci), (co, empty), (empty, empty)):
        assert plan(a, b) == 0 and cnt.value == 0
        assert L.giql_hip_contain_fill_dev(h, None, None, 0, st) == 0
        assert sum(eng.stats()["phase_launches"].values()) == 0
    # a chromosome id outside the dictionary
    bad = _side([0, 3], [0, 5], [9, 8]).c_struct()
    assert plan(bad, ci) == _lib.GIQL_ERR_CHROM
    assert fill()[0] == _lib.GIQL_ERR_STATE
    assert eng.contain_join(_side([], [], []), i, 1)[0].shape[0] == 0


def test_phase_bytes_cover_the_new_launches(eng):
    outer, inner, _ = _tile_case(CT_TILE + 1, 0, 0, 3)
    _contain(eng, outer, inner, 1, "general")
    st = eng.stats()
    assert st["phase_bytes"]["count"] >= 4 * (CT_TILE + 1) and st["phase_bytes"]["fill"] >= 4 * (CT_TILE + 1)
    assert st["phase_launches"]["count"] == 3 and st["phase_launches"]["fill"] == 1


# ------------------------------------------------------------------ the top of the axis, and past it
@pytest.mark.parametrize("which", ["default", "local"])
@pytest.mark.parametrize("name", ["tight_top", "one_chrom_max", "tight_over", "wide"])
def test_keys_at_the_top_of_the_axis_and_the_group_fallback(eng, eng_local, name, which):
    from giql_amd import _lib
    from test_axis_edges import FITS, LAYOUTS, dev, make_side, tight_span

    e = eng if which == "default" else eng_local
    enc = ("1based", "closed")
    a = make_side(name, enc, 1500, 1, irregular=60)
    b = make_side(name, enc, 2500, 2, irregular=60)
    n_chrom = len(LAYOUTS[name])
    da, db = dev(a), dev(b)
    if name in FITS:
        e.contain_plan(da, db, n_chrom)
        assert e.stats()["span"] == tight_span(name)
    else:
        with pytest.raises(_lib.GiqlHipError) as ei:
            e.contain_plan(da, db, n_chrom)
        assert ei.value.code == _lib.GIQL_ERR_SPAN
    for x, y, dx, dy in ((a, b, da, db), (b, a, db, da)):
        got = _pairs(*e.contain_join(dx, dy, n_chrom))
        want = R.contain_pairs(x.chrom, x.cs, x.ce, y.chrom, y.cs, y.ce)
        assert want.shape[0] > 50 and np.array_equal(got, want)
    if name in FITS:
        assert e.stats()["sort_local"] == (which == "local")


# ------------------------------------------------------------------ execute(): residuals, devices
def test_execute_with_residuals_beside_the_predicate(eng):
    from giql_amd.execute import execute
    from giql_amd.transpile import transpile

    case = max(CASES, key=lambda c: len(c["contains"]))
    assert tuple(case["enc_a"]) in R.OFFSETS
    from giql_amd.table import Table

    tables = [Table("ta", coordinate_system=case["enc_a"][0], interval_type=case["enc_a"][1]),
              Table("tb", coordinate_system=case["enc_b"][0], interval_type=case["enc_b"][1])]
    data = {"ta": _table(case["a"], 1), "tb": _table(case["b"], 2)}
    sa, sb = data["ta"].column("score").to_numpy(), data["tb"].column("score").to_numpy()
    plan = transpile("SELECT a.rid AS ra, b.rid AS rb FROM ta a JOIN tb b ON a.interval CONTAINS b.interval "
                     "AND a.score > b.score WHERE a.score >= 2 AND b.score < 5", tables, dialect="hip")
    ra, rb = execute(plan, data, eng, return_indices=True)
    want = [p for p in case["contains"] if sa[p[0]] > sb[p[1]] and sa[p[0]] >= 2 and sb[p[1]] < 5]
    assert 0 < len(want) < len(case["contains"])
    assert R.sort_pairs(np.stack([ra, rb], 1)).tolist() == want
    plan = transpile("SELECT a.rid AS ra, b.rid AS rb FROM ta a JOIN tb b ON a.interval WITHIN b.interval "
                     "AND a.score <= b.score", tables, dialect="hip")
    ra, rb = execute(plan, data, eng, return_indices=True)
    want = [p for p in case["within"] if sa[p[0]] <= sb[p[1]]]
    assert R.sort_pairs(np.stack([ra, rb], 1)).tolist() == want
    with pytest.raises(ValueError, match="WITHIN joins run on one device"):
        execute(plan, data, devices=[0, 0])
