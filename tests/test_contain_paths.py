"""CONTAINS / WITHIN on the GPU, kernel path by kernel path (contain_kernels.hip.h, giql_hip_contain_plan_dev_impl).

Every case comes from a seeded generator of ``tests/_contain_ref.py``; that a case reaches the path it is named after
is asserted from numpy restatements of the kernels' index arithmetic (``_contain_ref.reach``, run without a GPU by
``tests/test_contain.py::test_every_path_case_reaches_its_path``).  The truth is the O(n*m) brute force
``contain_pairs``; ``density-0.25`` alone (196,000 x 48,000 rows) takes the sort-based reference, which
``tests/test_contain.py`` anchors on the brute force.  Comparisons go through sorted pairs, ``stats()["n_out"]`` and
``stats()["join_form"]``; the general form's raw output is also held to the two properties its design gives whatever
the order of ties: the outer keys do not decrease over the regular pairs, and every pair with an irregular row lies
behind them.  Integers throughout: every comparison is exact."""

import ctypes
import functools

import numpy as np
import pytest

import _contain_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
C = R.constants()
SENTINEL = -7
PAD = 64


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


@pytest.fixture(scope="module")
def eng_general():
    """A context that runs the general form whatever the inner side's lengths."""
    e = _engine({"GIQL_HIP_NO_UNIFORM": "1"})
    yield e
    e.close()


def _side(cols):
    from giql_amd.engine import DeviceSide

    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.int32)).to(DEV)
    return DeviceSide(t(cols[0]), t(cols[1]), t(cols[2]), 0, 0)


@functools.lru_cache(maxsize=None)
def _sides(cid):
    case = R.path_case(cid)
    return _side(case.outer), _side(case.inner)


def _raw_order_holds(case, raw):
    """The general form's slots: the regular pairs first, in the order of the sorted outer side, then the pairs of
    the irregular rows."""
    (oc, os_, oe), (_ic, is_, ie) = case.outer, case.inner
    n_reg = case.regular_pairs().shape[0]
    head, tail = raw[:n_reg], raw[n_reg:]
    assert (oe > os_)[head[:, 0]].all() and (ie > is_)[head[:, 1]].all(), (case.id, "an irregular row among the regular pairs")
    key = oc[head[:, 0]].astype(np.int64) * (1 << 40) + os_[head[:, 0]]
    assert (np.diff(key) >= 0).all(), (case.id, "outer keys decrease over the regular pairs")
    assert ((oe <= os_)[tail[:, 0]] | (ie <= is_)[tail[:, 1]]).all(), (case.id, "a regular pair behind the irregular ones")


def _run(e, cid, form):
    case = R.path_case(cid)
    ro, ri = e.contain_join(*_sides(cid), case.n_chrom)
    st = e.stats()
    raw = np.stack([ro.cpu().numpy(), ri.cpu().numpy()], 1).astype(np.int64)
    want = case.want
    assert st["join_form"] == form, (cid, st["join_form"])
    assert st["n_out"] == raw.shape[0] == want.shape[0] > 0, (cid, st["n_out"], raw.shape, want.shape)
    assert np.array_equal(R.sort_pairs(raw), want), cid
    if form == "general":
        _raw_order_holds(case, raw)
    return st


# ---------------------------------------------------------------- the candidate tiles, path by path
@pytest.mark.parametrize("cid", R.GENERAL_PATHS)
def test_candidate_tile_path(eng, cid):
    """Density sweep (row owners per 64-candidate window from 63 down to 1, unstaged and staged tiles), a first tile
    of exactly CT_QCAP and CT_QCAP + 1 rows, a last tile pushed past the stage by trailing rows without candidates
    (regular ones past every inner start; irregular ones, which sort last), rows that enter the next tile as its row
    0 with lo > 0."""
    ev = R.reach(cid)
    print(f"\n[{cid}] " + ", ".join(f"{k}={v}" for k, v in ev.items()))
    _run(eng, cid, "general")


# ---------------------------------------------------------------- nothing is written past the total
def _raw_plan(e, cid):
    case = R.path_case(cid)
    o, i = _sides(cid)
    co, ci = o.c_struct(), i.c_struct()
    cnt = ctypes.c_int64(-1)
    rc = e._L.giql_hip_contain_plan_dev(e._h, ctypes.byref(co), ctypes.byref(ci), case.n_chrom, e._stream(), ctypes.byref(cnt))
    return rc, cnt.value


@pytest.mark.parametrize("cid, form", [("density-64", "general"), ("uniform-L2", "uniform_b"),
                                       ("trailing-irregular", "general")])
def test_the_fill_stays_inside_the_total(eng, cid, form):
    from giql_amd import _lib

    case = R.path_case(cid)
    want = case.want
    n = want.shape[0]
    assert _raw_plan(eng, cid) == (0, n) and eng.stats()["join_form"] == form
    assert (case.regular_pairs().shape[0] < n) == (cid == "trailing-irregular")      # irregular pairs behind the tiles'
    ro = torch.full((n + PAD,), SENTINEL, dtype=torch.int32, device=DEV)
    ri = torch.full((n + PAD,), SENTINEL, dtype=torch.int32, device=DEV)
    fill = lambda cap: eng._L.giql_hip_contain_fill_dev(eng._h, ro.data_ptr(), ri.data_ptr(), cap, eng._stream())
    assert fill(n - 1) == _lib.GIQL_ERR_CAPACITY
    torch.cuda.synchronize()
    assert int((ro != SENTINEL).sum()) == 0 and int((ri != SENTINEL).sum()) == 0, (cid, "a refused fill wrote")
    assert fill(n) == 0
    torch.cuda.synchronize()
    assert int((ro[n:] != SENTINEL).sum()) == 0 and int((ri[n:] != SENTINEL).sum()) == 0, (cid, "written past the total")
    assert int((ro[:n] == SENTINEL).sum()) == 0 and int((ri[:n] == SENTINEL).sum()) == 0, (cid, "a slot left unwritten")
    raw = np.stack([ro[:n].cpu().numpy(), ri[:n].cpu().numpy()], 1).astype(np.int64)
    assert np.array_equal(R.sort_pairs(raw), want), cid


# ---------------------------------------------------------------- the uniform form against the general form
@pytest.mark.parametrize("L", [1, 2, 150])
def test_uniform_form_against_the_general_form(eng, eng_general, L):
    """The same uniform-inner tables on a default context and on one that never takes the uniform form: both equal
    the brute force, hence each other.  The range count leaves its LDS window here (``reach``: 512-row outer tiles over
    more inner keys than the window stages, rows ending past a window that holds their tile's whole range, short rows
    starting past it, the upper key clamped at 0 for L = 150)."""
    cid = f"uniform-L{L}"
    ev = R.reach(cid)
    print(f"\n[{cid}] " + ", ".join(f"{k}={v}" for k, v in ev.items()))
    _run(eng, cid, "uniform_b")
    _run(eng_general, cid, "general")


# ---------------------------------------------------------------- the sorts under CONTAINS
LOCAL = {"GIQL_HIP_LOCAL_MIN_ROWS": "1"}
FORMS = {   # name -> (environment, three-stage sort expected, bucket bits)
    "local": (LOCAL, True, 16),
    "local13": ({**LOCAL, "GIQL_HIP_LOCAL_BITS": "13"}, True, 13),
    "local14": ({**LOCAL, "GIQL_HIP_LOCAL_BITS": "14"}, True, 14),
    "local15": ({**LOCAL, "GIQL_HIP_LOCAL_BITS": "15"}, True, 15),
    "no_local": ({**LOCAL, "GIQL_HIP_NO_LOCAL_SORT": "1"}, False, None),
}


def test_sorts_under_every_form():
    """(key, end, rid) for the outer side and, in the uniform form, (key, rid) without an ``end`` column for the inner
    one, through the three-stage sort at every bucket width the project accepts and through the four global passes."""
    met = set()
    for form, (env, local, bits) in FORMS.items():
        e = _engine(env)
        try:
            for cid, join_form in (("sort-general", "general"), ("sort-uniform", "uniform_b")):
                R.reach(cid)
                st = _run(e, cid, join_form)
                assert st["sort_local"] == local and not st["sort_resorted"], (form, cid, st)
                if bits is not None:
                    assert st["bucket_bits"] == bits, (form, cid, st["bucket_bits"])
                assert st["span"] > 0 and st["sort_order_fallbacks"] == 0
                met.add((cid, st["sort_local"], st["bucket_bits"] if st["sort_local"] else None))
        finally:
            e.close()
    print(f"\n[sort forms] (case, three-stage sort, bucket bits) met: {sorted(met, key=str)}")
    for cid in ("sort-general", "sort-uniform"):
        assert {f[1] for f in met if f[0] == cid} == {True, False}, met
        assert {f[2] for f in met if f[0] == cid} == {13, 14, 15, 16, None}, met


# ---------------------------------------------------------------- the repeat in ticket order
def test_an_injected_timeout_repeats_the_plan_in_ticket_order():
    """GIQL_HIP_INJECT_TIMEOUT=1: the first clean read-back of the context (contain_plan's read of the spans) reports
    a look-back timeout, ``with_order_fallback`` repeats the plan in ticket order, and the context stays in it."""
    e = _engine({"GIQL_HIP_INJECT_TIMEOUT": "1"})
    try:
        assert e.stats()["sort_tile_order"] == 2
        st = _run(e, "density-64", "general")
        assert (st["sort_tile_order"], st["sort_order_fallbacks"]) == (0, 1), st
        st = _run(e, "uniform-L2", "uniform_b")
        assert (st["sort_tile_order"], st["sort_order_fallbacks"]) == (0, 1), st       # no further repeat
    finally:
        e.close()
