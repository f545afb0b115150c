"""LEFT OUTER joins on the GPU: the pad kernels (giql_hip_left_pad_dev) against numpy, HipEngine.left_join against
the oracle's pairs + setdiff1d, execute() against SQLite running the same LEFT JOIN with the predicate spelt out.
Needs a GPU."""

from dataclasses import replace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

pa = pytest.importorskip("pyarrow")
torch = pytest.importorskip("torch")

import _left_ref as R  # noqa: E402
from giql_amd import _lib, synth  # noqa: E402
from giql_amd.engine import LEFT_PAD_BLOCK_ROWS as B, DeviceSide  # noqa: E402
from giql_amd.execute import execute, pin  # noqa: E402
from giql_amd.plan import Aggregate  # noqa: E402
from giql_amd.transpile import build_plan, transpile  # noqa: E402
from oracle import pyoracle as ora  # noqa: E402

SENTINEL = -7            # what the buffers hold where nothing may be written
MAX_PAIRS = 300_000


@pytest.fixture(scope="module")
def eng():
    from giql_amd.engine import HipEngine

    e = HipEngine(0)
    yield e
    e.close()


def to_dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to("cuda:0")


def dev(s: ora.Side) -> DeviceSide:
    return DeviceSide.from_numpy(s.chrom, s.start, s.end)


# ------------------------------------------------------------------------------------------------ left_pad
def pad_buffers(ids, room, with_b=True):
    ids = np.asarray(ids, np.int32)
    n = ids.size
    row_a = np.full(n + room, SENTINEL, np.int32)
    row_a[:n] = ids
    row_b = np.full(n + room, SENTINEL, np.int32)
    row_b[:n] = np.arange(n) % 5
    return to_dev(row_a), (to_dev(row_b) if with_b else None), row_b


def check_pad(eng, ids, n_rows, with_b=True, slack=3, what=""):
    """One left_pad call over ``ids`` with ``slack`` entries more room than needed, checked entry by entry."""
    ids = np.asarray(ids, np.int32)
    n = ids.size
    want = R.pad_ids(ids, n_rows)
    row_a, row_b, b_before = pad_buffers(ids, want.size + slack, with_b)
    total = eng.left_pad(row_a, row_b, n, n_rows)
    assert total == n + want.size == eng.last_total, what
    ga = row_a.cpu().numpy()
    assert np.array_equal(ga[:n], ids), what                      # the pairs stay as they are
    assert np.array_equal(ga[n:total], want), what                # the unmatched rows, ascending
    assert (ga[total:] == SENTINEL).all(), what                   # nothing past them
    if with_b:
        gb = row_b.cpu().numpy()
        assert np.array_equal(gb[:n], b_before[:n]), what
        assert (gb[n:total] == -1).all() and (gb[total:] == SENTINEL).all(), what
    if n_rows:
        assert eng.stats()["n_out"] == total, what
    return want.size


def runs(rng, n_rows, n_pairs):
    """Ids as a join leaves them: runs of one left row, the rows in no particular order."""
    rows = rng.choice(n_rows, size=max(1, min(n_rows * 3 // 4, n_pairs // 4)), replace=False)
    reps = rng.integers(1, 8, size=rows.size)
    return np.repeat(rows, reps)[:n_pairs]


@pytest.mark.parametrize("n_rows", [0, 1, 31, 32, 33, B - 1, B, B + 1, 3 * B + 17, 1_000_003])
def test_left_pad_against_numpy(eng, n_rows):
    rng = np.random.default_rng(n_rows)
    assert check_pad(eng, [], n_rows, what="no pairs") == n_rows                  # every row is appended
    assert check_pad(eng, [], n_rows, with_b=False, what="no pairs, ids only") == n_rows
    if n_rows == 0:
        return
    one = np.full(1000, n_rows // 2)
    assert check_pad(eng, one, n_rows, what="all pairs on one row") == n_rows - 1
    mixed = runs(rng, n_rows, MAX_PAIRS)
    n_pad = check_pad(eng, mixed, n_rows, what="runs")
    assert n_rows <= 33 or 0 < n_pad < n_rows
    check_pad(eng, mixed, n_rows, with_b=False, slack=0, what="runs, ids only, exact room")
    check_pad(eng, rng.permutation(mixed), n_rows, what="the same ids in no order")
    if n_rows <= MAX_PAIRS:
        every = rng.permutation(n_rows)
        assert check_pad(eng, every, n_rows, what="every row matched") == 0        # nothing is appended
        assert check_pad(eng, np.sort(every), n_rows, slack=0, what="every row matched, sorted, exact room") == 0
        assert check_pad(eng, rng.permutation(n_rows - 1), n_rows, what="only the last row unmatched") == 1
        assert check_pad(eng, 1 + rng.permutation(n_rows - 1), n_rows, what="only row 0 unmatched") == 1
        assert check_pad(eng, np.repeat(every, 2), n_rows, with_b=False, what="every row twice") == 0


@pytest.mark.parametrize("n_rows", [33, B + 1, 3 * B + 17])
def test_left_pad_short_capacity_reports_the_size_and_writes_nothing(eng, n_rows):
    rng = np.random.default_rng(7 + n_rows)
    ids = runs(rng, n_rows, 5000)
    want = R.pad_ids(ids, n_rows)
    assert want.size > 1
    for room in (0, want.size - 1):
        row_a, row_b, b_before = pad_buffers(ids, room)
        with pytest.raises(_lib.GiqlHipError) as exc:
            eng.left_pad(row_a, row_b, ids.size, n_rows)
        assert exc.value.code == _lib.GIQL_ERR_CAPACITY
        assert eng.last_total == ids.size + want.size
        ga, gb = row_a.cpu().numpy(), row_b.cpu().numpy()
        assert np.array_equal(ga[:ids.size], ids) and (ga[ids.size:] == SENTINEL).all()
        assert np.array_equal(gb, b_before)
    check_pad(eng, ids, n_rows, slack=0, what="the repeat call with enough room")


@pytest.mark.parametrize("bad_of", [lambda n: n, lambda n: -1, lambda n: n + B, lambda n: -(2 ** 31)])
def test_left_pad_rejects_an_id_outside_the_table(eng, bad_of):
    n_rows = B + 5
    rng = np.random.default_rng(3)
    ids = runs(rng, n_rows, 4000).astype(np.int64)
    ids[ids.size // 2] = bad_of(n_rows)
    row_a, row_b, b_before = pad_buffers(ids, n_rows)
    with pytest.raises(_lib.GiqlHipError) as exc:
        eng.left_pad(row_a, row_b, ids.size, n_rows)
    assert exc.value.code == _lib.GIQL_ERR_INVALID and "outside" in str(exc.value)
    assert (row_a.cpu().numpy()[ids.size:] == SENTINEL).all()      # nothing appended
    assert np.array_equal(row_b.cpu().numpy(), b_before)
    check_pad(eng, runs(rng, n_rows, 4000), n_rows, what="the context goes on working")


def test_left_pad_checks_its_arguments(eng):
    row_a = to_dev(np.zeros(8))
    with pytest.raises(ValueError):
        eng.left_pad(row_a, None, 9, 4)                             # more pairs than the buffer holds
    with pytest.raises(ValueError):
        eng.left_pad(row_a, to_dev(np.zeros(4)), 5, 4)              # (the shorter buffer counts)
    with pytest.raises(_lib.GiqlHipError) as exc:
        eng.left_pad(row_a, None, 0, 2 ** 31)
    assert exc.value.code == _lib.GIQL_ERR_INVALID


# ----------------------------------------------------------------------------------------------- left_join
def table(n, seed, kind, chroms=None):
    return ora.Side(*synth.make_table(n, seed, kind, chroms=chroms))


@pytest.fixture(scope="module")
def left_table():
    return table(50_000, 21, "peaks")


@pytest.mark.parametrize("kind_b,chroms_b", [("reads", None), ("peaks", None), ("reads", range(0, 24, 2))])
def test_left_join_against_the_numpy_restatement(eng, left_table, kind_b, chroms_b):
    a = left_table
    b = table(300_000, 11, kind_b, chroms=chroms_b)
    want = R.left_rows(a, b)
    n_pad = int((want[:, 1] < 0).sum())
    assert 0 < n_pad < a.n and want.shape[0] > a.n               # matched and unmatched rows, some rows matched twice
    if chroms_b is not None:                                      # whole chromosomes of the left table have no partner
        assert set(np.unique(a.chrom)) - set(np.unique(b.chrom))
    for call in range(2):     # (the second call sizes its buffers from the first: the one-call join)
        ra, rb = eng.left_join(dev(a), dev(b), 24)
        assert ra.dtype == torch.int32 and rb.dtype == torch.int32
        ga, gb = ra.cpu().numpy(), rb.cpu().numpy()
        assert np.array_equal(R.sort_rows(ga, gb), want), call
        n_pairs = ga.size - n_pad
        assert (gb[:n_pairs] >= 0).all() and (gb[n_pairs:] == -1).all(), call
        assert np.array_equal(ga[n_pairs:], R.pad_ids(ga[:n_pairs], a.n)), call      # the padded rows, ascending


def test_left_join_keeps_its_room_when_the_pair_count_outgrows_the_guess():
    """Two table pairs of equal row counts on one engine: the second join's buffers are sized from the first one's
    pair count.  100 pairs then 5000 (on five left rows, 995 rows to pad): 5000 pairs fit the guessed buffers only
    by spending the room kept for the pad, which must therefore never be offered to the join."""
    from giql_amd.engine import HipEngine

    def side(start, length):
        start = np.asarray(start, np.int32)
        return ora.Side(np.zeros(start.size, np.int32), start, start + np.asarray(length, np.int32))

    k = np.arange(1000)
    a1, b1 = side(k * 1000, 10), side(np.where(k < 100, k * 1000 + 5, 2_000_000 + k * 1000), 10)
    a2 = side(np.where(k < 5, 0, 3_000_000 + k * 1000), np.where(k < 5, 1_500_000, 10))     # five rows span all of b2
    b2 = side(k * 1000 + 7, 10)
    want1, want2 = R.left_rows(a1, b1), R.left_rows(a2, b2)
    assert (want1[:, 1] >= 0).sum() == 100 and (want2[:, 1] >= 0).sum() == 5000 and (want2[:, 1] < 0).sum() == 995
    e = HipEngine(0)
    try:
        for a, b, want in ((a1, b1, want1), (a2, b2, want2), (a1, b1, want1), (a2, b2, want2)):
            ra, rb = e.left_join(dev(a), dev(b), 1)
            assert np.array_equal(R.sort_rows(ra.cpu().numpy(), rb.cpu().numpy()), want)
            ja, jb = e.inner_join(dev(a), dev(b), 1)       # (the INNER join shares the buffer logic)
            assert np.array_equal(R.sort_rows(ja.cpu().numpy(), jb.cpu().numpy()), want[want[:, 1] >= 0])
    finally:
        e.close()


def test_left_join_with_an_empty_side(eng, left_table):
    a, none = left_table, ora.Side(*(np.zeros(0, np.int32),) * 3)
    ra, rb = eng.left_join(dev(a), dev(none), 24)
    assert np.array_equal(ra.cpu().numpy(), np.arange(a.n)) and (rb.cpu().numpy() == -1).all()
    ra, rb = eng.left_join(dev(none), dev(a), 24)
    assert ra.numel() == 0 and rb.numel() == 0


# ------------------------------------------------------------------------------------------------ execute()
@pytest.fixture(scope="module")
def tables():
    return R.make_tables()


COLS, FROM, CASES = R.COLS, R.FROM, R.CASES
PREDICATE_CASES = {
    "contains": "a.interval CONTAINS b.interval",
    "within": "a.interval WITHIN b.interval",
    "distance": "DISTANCE(a.interval, b.interval) <= 40",
}


def run_both(template, tables, eng, predicate=R.INTERSECTS):
    """execute() with both projection settings and SQLite over one template -> (rows, rows, rows, last Arrow table)."""
    giql, sql = R.giql_and_sql(template, predicate)
    plan = transpile(giql, ["peaks", "genes"], dialect="hip", outer_joins=True)
    got = []
    for device_projection in (True, False):
        out = execute(plan, tables, eng, device_projection=device_projection)
        got.append([tuple(r.values()) for r in out.to_pylist()])
    return got[0], got[1], R.sqlite_rows(tables, sql), out


@pytest.mark.parametrize("case", sorted(CASES))
def test_execute_against_sqlite(eng, tables, case):
    dev_rows, host_rows, want, _ = run_both(CASES[case], tables, eng)
    assert want, case
    assert R.bag(dev_rows) == R.bag(want), case
    assert R.bag(host_rows) == R.bag(want), case


@pytest.mark.parametrize("name", sorted(PREDICATE_CASES))
def test_execute_other_predicates_against_sqlite(eng, tables, name):
    template = f"SELECT {COLS} {FROM} AND a.score > 1 WHERE b.score IS NULL OR b.score < 10"
    dev_rows, host_rows, want, _ = run_both(template, tables, eng, PREDICATE_CASES[name])
    assert any(r[4] is None for r in want) and any(r[4] is not None for r in want), name
    assert R.bag(dev_rows) == R.bag(want) and R.bag(host_rows) == R.bag(want), name


def test_execute_count_over_a_right_column_skips_the_padded_rows(eng, tables):
    # COUNT(b.name) beside the others: the front end keeps a COUNT(<right column>) item for the count_overlaps gate,
    # so the aggregate is added to the lowered plan by hand -- execute() is what is checked here
    template = f"SELECT a.chrom, COUNT(*) AS n, SUM(b.score) AS s {FROM} GROUP BY a.chrom"
    giql, sql = R.giql_and_sql(template)
    plan = build_plan(giql, ["peaks", "genes"], outer_joins=True)
    plan = replace(plan, aggregates=plan.aggregates + (Aggregate("COUNT", "r", "name", "nb"),), output=plan.output + ("nb",))
    want = R.sqlite_rows(tables, sql.replace("SUM(b.score) AS s", "SUM(b.score) AS s, COUNT(b.name) AS nb"))
    assert any(r[1] > r[3] for r in want)
    for device_projection in (True, False):
        out = execute(plan, tables, eng, device_projection=device_projection)
        assert out.column_names == ["chrom", "n", "s", "nb"]
        assert R.bag(tuple(r.values()) for r in out.to_pylist()) == R.bag(want)


@pytest.mark.parametrize("order", ["b.score NULLS FIRST, a.start, a.name, b.start",
                                   "b.score DESC NULLS LAST, a.start DESC, a.name, b.start",
                                   "b.score NULLS LAST, a.start, a.name NULLS LAST, b.start",
                                   "b.score DESC NULLS FIRST, a.start, a.name, b.start"])
def test_execute_order_by_a_right_column_and_limit(eng, tables, order):
    template = f"SELECT a.name, a.start, b.score AS b_score, b.start AS b_start {FROM} ORDER BY {order} LIMIT 40"
    dev_rows, host_rows, want, _ = run_both(template, tables, eng)
    assert len(want) == 40
    assert dev_rows == want and host_rows == want      # (rows that tie on every key are equal rows)


def test_execute_right_columns_are_null_on_padded_rows(eng, tables):
    for device_projection in (True, False):
        giql, sql = R.giql_and_sql(CASES["loj"])
        out = execute(transpile(giql, ["peaks", "genes"], dialect="hip", outer_joins=True), tables, eng,
                      device_projection=device_projection)
        want = R.sqlite_rows(tables, sql)
        assert out.schema.field("b_name").type == pa.string() and out.schema.field("b_big").type == pa.int64()
        assert out.schema.field("b_start").type == pa.int32()
        for i, name in ((3, "b_name"), (4, "b_start"), (5, "b_score"), (6, "b_big")):
            col = out.column(name)
            assert col.null_count == sum(r[i] is None for r in want) > 0, name
            assert sorted(v for v in col.to_pylist() if v is not None) == sorted(r[i] for r in want if r[i] is not None), name
        n_pad = out.column("b_start").null_count          # (genes.start has no NULLs of its own)
        assert out.column("b_name").null_count > n_pad and out.column("b_big").null_count > n_pad
        assert out.column("start").null_count == 0        # a left column is never NULL because of padding


def test_execute_return_indices(eng, tables):
    giql, _ = R.giql_and_sql(CASES["loj"])
    plan = build_plan(giql, ["peaks", "genes"], outer_joins=True)
    ra, rb = execute(plan, tables, eng, return_indices=True)
    names = sorted(set(tables["peaks"]["chrom"].to_pylist()) | set(tables["genes"]["chrom"].to_pylist()))
    side = lambda t: ora.Side(np.array([names.index(c) for c in t["chrom"].to_pylist()], np.int32),  # noqa: E731
                              t["start"].to_numpy().astype(np.int32), t["end"].to_numpy().astype(np.int32))
    want = R.left_rows(side(tables["peaks"]), side(tables["genes"]))
    assert np.array_equal(R.sort_rows(ra, rb), want)
    assert (want[:, 1] == -1).any() and (np.asarray(rb) == -1).sum() == (want[:, 1] == -1).sum()
    # a WHERE that drops every padded row leaves no -1 behind
    giql, _ = R.giql_and_sql(CASES["where_right"])
    ra, rb = execute(build_plan(giql, ["peaks", "genes"], outer_joins=True), tables, eng, return_indices=True)
    assert len(rb) and (np.asarray(rb) >= 0).all()


def test_execute_takes_a_query_string_with_the_switch(eng, tables):
    giql, sql = R.giql_and_sql(CASES["where_or_mixed"])
    out = execute(giql, tables, eng, giql_tables=["peaks", "genes"], outer_joins=True)
    assert R.bag(tuple(r.values()) for r in out.to_pylist()) == R.bag(R.sqlite_rows(tables, sql))
    from giql_amd.transpile import HipDeclined

    with pytest.raises(HipDeclined):
        execute(giql, tables, eng, giql_tables=["peaks", "genes"])


def test_execute_with_an_empty_right_table(eng, tables):
    giql, sql = R.giql_and_sql(CASES["where_or_with_null_test"])
    t = {"peaks": tables["peaks"], "genes": tables["genes"].slice(0, 0)}
    plan = transpile(giql, ["peaks", "genes"], dialect="hip", outer_joins=True)
    for device_projection in (True, False):
        out = execute(plan, t, eng, device_projection=device_projection)
        assert out.num_rows == tables["peaks"].num_rows and out.column("b_name").null_count == out.num_rows
        assert R.bag(tuple(r.values()) for r in out.to_pylist()) == R.bag(R.sqlite_rows(t, sql))


# ------------------------------------------------------------------------------------------------- routing
def test_left_plans_run_on_one_device(eng, tables):
    giql, _ = R.giql_and_sql(CASES["loj"])
    plan = build_plan(giql, ["peaks", "genes"], outer_joins=True)
    with pytest.raises(NotImplementedError, match="one device"):
        execute(plan, tables, devices=[0, 0])
    assert execute(plan, tables, devices=[0]).num_rows == execute(plan, tables, eng).num_rows


def test_pinned_tables_take_the_ordinary_path(eng, tables):
    giql, sql = R.giql_and_sql(CASES["on_and_where"])
    plan = build_plan(giql, ["peaks", "genes"], outer_joins=True)
    with pin(tables["peaks"]) as p, pin(tables["genes"], index=True) as g:
        out = execute(plan, {"peaks": p, "genes": g}, eng)
        assert not g.index_info()                      # no index was built for it
    assert R.bag(tuple(r.values()) for r in out.to_pylist()) == R.bag(R.sqlite_rows(tables, sql))
