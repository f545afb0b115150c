"""Every device entry point on a side stream, behind pending work -- the GPU part needs a GPU.

``HipEngine`` hands ``torch.cuda.current_stream()`` to every ``*_dev`` entry point, and the rest of the suite runs on
the null stream, where a launch, a memset or a synchronisation on the wrong stream cannot be seen.  Here every case
(tests/_stream_harness.py: ``CASES``) runs on one ``torch.cuda.Stream()`` ``s`` under the stale / fresh protocol:

1. the input buffers hold ``STALE``, the ``FRESH`` staging tensors are uploaded, ``torch.cuda.synchronize()``;
2. under ``s``: a bounded delay (``torch.cuda._sleep``);
3. ``buf.copy_(fresh, non_blocking=True)`` for every input buffer, device to device;
4. the call, through its ``HipEngine`` method (a plan and its fill: both);
5. a clone of every input buffer;
6. ``STALE`` copied back over every input buffer -- a legal, stream-ordered reuse by the caller;
7. only then the results come to the host.

The result must be ``reference(FRESH)`` by the operator's own comparison rule (pairs as sorted multisets, NEAREST rows
by distance and the matched row's (start, end), float SUM / AVG within the derived bound of
test_merge_aggregates_gpu.py, everything else exactly), the clones must be ``FRESH`` bit for bit (no input was
written), and the same holds for a second run on the same context, which starts from the context's guesses.  Both
input sets are valid for their operator and share every shape, row count and id range, so work that runs out of
order computes a wrong answer, never an out-of-range access.

The delay, measured on an MI355X (warm contexts, the default stream): the slowest call sequence of a case takes
``t_host`` = 2.4 ms of host time (``merge_agg[wide]``: three ABI calls per chromosome group and torch indexing between
them; ``inner_join[wide]`` 1.6 ms, every other case under 0.8 ms) and the slowest ``execute()`` query below 2.1 ms.
The cases of the pair aggregates and of coverage, measured the same way when they were added, stay under that:
``coverage[wide]`` 0.93 ms (``merge_agg[wide]`` 1.45 ms and ``inner_join[wide]`` 1.14 ms in that run), ``pair_aggregate``
0.29 ms, ``pair_aggregate[expr]`` 0.27 ms, the three one-call coverage cases 0.16 ms; their ``execute()`` queries
1.81 ms (join aggregates), 1.42 ms (aggregate expressions) and 0.48 ms (coverage).  ``t_host`` stays 2.4 ms.
The delay ``D`` is 40 ms -- at least ``2 * t_host``, at least 20 ms, under the cap of 200 ms -- and
``torch.cuda._sleep`` counts 2.4 million cycles per millisecond there.  The fixtures calibrate that with event pairs at
every run, ask for a quarter more than ``D`` and check what they get with another pair on ``s``: 50.0 ms.

Two controls show that the protocol has teeth in the process it runs in.  A clone issued under the default stream
right after step 3 still reads ``STALE`` (null-stream work overtakes ``s``), and ``count_overlaps`` with
``HipEngine._stream`` patched to return the null stream answers from ``STALE`` rows.  The first needs care in the
choice of ``s``: the runtime spreads the streams of a process over four hardware queues, every fourth new stream
shares the null stream's queue (measured: of twelve streams made in a row, the default stream overtook all but
every fourth), and on such a stream null-stream work waits behind the delay.  With the whole suite in one process the
first ``torch.cuda.Stream()`` of this file was such a stream and both controls failed; the ``side`` fixture now asks
the device, per candidate, whether the default stream overtakes it.

Which cases fork the context's second stream (``SideChain``, giql_hip.hip): the INNER plan, SEMI / ANTI, COUNT and
NEAREST k = 1 do, for a smaller side of at most ``OVERLAP_MAX_ROWS`` = 4M rows that is not sorted in three stages
(``sort_is_local``).  On the default engine (``sort_is_local`` is false below 2^21 rows) that is every ``inner_*``,
``left_join``, ``semi_join``, ``anti_join``, ``count_overlaps``, ``nearest[...]`` and ``nearest32`` case here:
``SideChain`` is active.  The ``...@local`` cases run the same calls on a context made with
``GIQL_HIP_LOCAL_MIN_ROWS=1``, where every side is sorted in three stages and ``SideChain`` stays inactive.

The stated limit: the delay orders only what a call issues before its first synchronisation of ``s`` -- after that
the copies of step 3 have landed.  Steps 5 and 6 cover the tail (work that still reads the inputs after the call
returned); the middle of a call of several phases is covered only where a later phase reads the inputs again.
"""

import ctypes

import numpy as np
import pytest

import _stream_harness as H

gpu = pytest.mark.gpu

DELAY_MS = 40.0          # D: see the module docstring
DELAY_CAP_MS = 200.0


# ================================================================================================ CPU
def test_every_stream_entry_point_has_a_case():
    """Every symbol of ``_lib`` whose declaration takes a stream maps to a case; the two probes are the only
    exemptions: they return one bandwidth figure, which has no checkable value."""
    declared = H.stream_entry_points()
    symbols = H.abi_symbols()      # every ``..._SYMBOLS`` list of ``_lib``, found by name
    assert len(symbols) == len(set(symbols))
    assert set(declared) <= set(symbols) and len(declared) == len(set(declared))
    assert sum(s.endswith("_dev") for s in symbols) == len(declared)      # (every *_dev entry point takes one)
    covered = {}
    for c in H.CASES.values():
        for name in c.symbols:
            covered.setdefault(name, []).append(c.id)
    names = [H.short(s) for s in declared]
    assert set(covered) <= set(names), sorted(set(covered) - set(names))
    assert H.NO_CHECKABLE_OUTPUT == ("copy_probe", "stream_probe") and not set(H.NO_CHECKABLE_OUTPUT) & set(covered)
    missing = [n for n in names if n not in covered and n not in H.NO_CHECKABLE_OUTPUT]
    assert not missing, f"entry points that take a stream and have no case in tests/_stream_harness.py: {missing}"


@pytest.mark.parametrize("cid", list(H.CASES))
def test_stale_and_fresh_are_two_valid_inputs_with_two_answers(cid):
    c = H.CASES[cid]
    stale, fresh = c.inputs("stale"), c.inputs("fresh")
    assert sorted(stale) == sorted(fresh)
    for k in stale:
        assert stale[k].shape == fresh[k].shape and stale[k].dtype == fresh[k].dtype, k
        assert not H.bitwise_equal(stale[k], fresh[k]), k
    for inp in (stale, fresh):
        for k in inp:
            if k.endswith(".start"):      # start <= end where NEAREST, CLUSTER, MERGE, DISJOIN and DISTANCE need it
                assert np.all(inp[k] <= inp[k[:-6] + ".end"]), k
    assert not H.same(H.exact_part(c.want("stale")), H.exact_part(c.want("fresh")))


def test_ids_and_offsets_stay_inside_their_tables():
    """What keeps a torn read (one buffer FRESH, its neighbour STALE) inside its allocation."""
    for which in ("stale", "fresh"):
        for cid, names, n_rows in (("take[vector]", ["idx"], H.TAKE_ROWS), ("select", ["ia", "ib"], H.TAKE_ROWS),
                                   ("mark", ["idx"], H.MARK_ROWS), ("segment_sum", ["gid"], H.SEG_GROUPS),
                                   ("left_pad_pairs", ["ra"], H.PAD_ROWS), ("take_utf8", ["idx"], len(H.UTF8_LENGTHS))):
            inp = H.CASES[cid].inputs(which)
            for k in names:
                assert inp[k].min() >= -1 and inp[k].max() < n_rows, (cid, k)
        for cid in ("pair_aggregate", "pair_aggregate[expr]"):      # pair ids: no -1, the kernel refuses one
            inp = H.CASES[cid].inputs(which)
            assert inp["ra"].shape == inp["rb"].shape == (H.PAGG_PAIRS,), cid
            assert inp["ra"].min() >= 0 and inp["ra"].max() < H.PAGG_NA and inp["rb"].min() >= 0 and inp["rb"].max() < H.PAGG_NB, cid
            assert inp["ca"].shape == inp["ca.valid"].shape == (H.PAGG_NA,), cid        # columns as long as their table
            assert all(inp[k].shape == (H.PAGG_NB,) for k in ("vf", "vf.valid", "vi")), cid
            assert np.bincount(inp["ra"], minlength=H.PAGG_NA).min() > 0, cid            # every A row has pairs
        plan = H.CASES["fill_from_plan"].inputs(which)
        assert plan["lo"].min() >= 0 and plan["lo"].max() + H.PLAN_MAX_CNT <= H.PLAN_NS and plan["cnt"].max() < H.PLAN_MAX_CNT
        for cid, off, data in (("take_utf8", "off", "data"), ("merge_agg[STRING_AGG]", "w.off", "w.data")):
            inp = H.CASES[cid].inputs(which)
            assert inp[off][0] == 0 and np.all(np.diff(inp[off]) >= 0) and inp[off][-1] == inp[data].shape[0], cid
    for cid, off in (("take_utf8", "off"), ("merge_agg[STRING_AGG]", "w.off")):      # equal bytes in all: any mix fits
        assert H.CASES[cid].inputs("stale")[off][-1] == H.CASES[cid].inputs("fresh")[off][-1]
    assert sorted(set(np.diff(H.CASES["take_utf8"].inputs("fresh")["off"]))) == [0, 31, 32, 33, 300]


def _fake_case(null_stream):
    """``out = 2 * x`` as an entry point launches it: on the caller's stream, or (mis-streamed) on the null stream."""
    be = H.FakeBackend()
    s = H.FakeStream(be)
    stale, fresh = {"x": np.arange(8, dtype=np.int64)}, {"x": np.arange(8, dtype=np.int64) * 10 + 1}

    def call(bufs):
        out = H.FakeTensor(np.zeros(8, np.int64))

        def kernel():
            out.arr[...] = 2 * bufs["x"].arr
        be.launch(kernel, null_stream=null_stream)
        return out, 7

    (out, seven), clones = H.run_protocol(be, s, stale, fresh, call, 1000)
    assert seven == 7 and not s.queue
    return be, out, clones, stale, fresh


def test_the_protocol_on_a_model_of_stream_order():
    """The harness's own ordering, on the host: uploads, one device synchronisation, then on the side stream the
    delay, the FRESH copies, the call, the clones, the STALE copies, and only then a read; the stream's own
    synchronisation comes last.  A call in stream order answers from FRESH and leaves FRESH behind."""
    be, out, clones, _stale, fresh = _fake_case(null_stream=False)
    steps = [w for w, _where in be.log]
    assert steps == ["upload"] * 3 + ["synchronize", "sleep", "copy", "launch", "clone", "copy", "to_host", "to_host",
                                      "stream_synchronize"]
    assert all(where == "side" for _w, where in be.log[4:])
    assert np.array_equal(out, 2 * fresh["x"]) and np.array_equal(clones["x"], fresh["x"])


def test_the_protocol_catches_a_launch_on_the_null_stream_on_the_model():
    be, out, clones, stale, fresh = _fake_case(null_stream=True)
    assert ("launch", "default") in be.log
    assert np.array_equal(out, 2 * stale["x"]) and not np.array_equal(out, 2 * fresh["x"])
    assert np.array_equal(clones["x"], fresh["x"])


def test_control_one_on_the_model():
    be = H.FakeBackend()
    s = H.FakeStream(be)
    stale, fresh = {"x": np.arange(5)}, {"x": np.arange(5) + 100}
    early, late = H.control_clones(be, s, stale, fresh, 1000)
    assert np.array_equal(early["x"], stale["x"]) and np.array_equal(late["x"], fresh["x"]) and not s.queue


def test_same_compares_by_the_rule_of_the_leaf():
    a = np.array([1.0, 2.0])
    assert H.same((a, 3, None, b"x"), (a.copy(), 3, None, b"x")) and not H.same((a,), (a + 1e-12,))
    assert H.same(a + 1e-12, H.Approx(a, [1e-11, 1e-11])) and not H.same(a + 1e-10, H.Approx(a, [1e-11, 1e-11]))
    assert not H.same(np.zeros(3), np.zeros(4)) and not H.same((a,), (a, a))
    assert H.same(np.array([1, 2], np.int32), np.array([1, 2], np.int64))


# ================================================================================================ GPU
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def be():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return H.TorchBackend()


@pytest.fixture(scope="module")
def engines(monkeypatch_module):
    from giql_amd.engine import HipEngine

    monkeypatch_module.delenv("GIQL_HIP_LOCAL_MIN_ROWS", raising=False)
    default = HipEngine(0)
    monkeypatch_module.setenv("GIQL_HIP_LOCAL_MIN_ROWS", "1")      # every side sorted in three stages: no SideChain
    local = HipEngine(0)
    monkeypatch_module.delenv("GIQL_HIP_LOCAL_MIN_ROWS")
    yield {"default": default, "local": local}
    torch.cuda.synchronize()
    default.close()
    local.close()


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


def _timed_sleep(s, cycles):
    """Milliseconds ``torch.cuda._sleep(cycles)`` holds ``s``, by an event pair on ``s``."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        e0.record()
        torch.cuda._sleep(int(cycles))
        e1.record()
    s.synchronize()
    return e0.elapsed_time(e1)


@pytest.fixture(scope="module")
def cycles_per_ms(be):
    """What ``torch.cuda._sleep`` counts in a millisecond, by event pairs on a stream of its own."""
    s = torch.cuda.Stream()
    _timed_sleep(s, 1000)                        # (the first launch pays for loading the kernel)
    probe = 1_000_000
    ms = _timed_sleep(s, probe)
    while ms < 5.0 and probe < 1 << 36:          # a bounded spin every time: at most a few doublings
        probe *= 4
        ms = _timed_sleep(s, probe)
    # the counter follows the shader clock: the fastest of three probes (and a quarter more, below) keeps the delay at
    # or above D whatever the clock does afterwards; a slower clock only lengthens it, and the cap leaves room for 4x
    return max(probe / ms, *(probe / _timed_sleep(s, probe) for _ in range(2)))


def _overtakes(s, cycles):
    """Does work on the default stream finish while ``s`` is still inside a delay?  Asked of the device itself: an
    event behind the delay on ``s`` must still be pending when one behind a small default-stream kernel is done."""
    x = torch.zeros(64, device="cuda:0")
    torch.cuda.synchronize()
    behind_delay, behind_kernel = torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(s):
        torch.cuda._sleep(int(cycles))
        behind_delay.record()
    x.add_(1)
    behind_kernel.record()
    behind_kernel.synchronize()
    still_pending = not behind_delay.query()
    s.synchronize()
    return still_pending


@pytest.fixture(scope="module")
def side(be, cycles_per_ms):
    """The side stream ``s``.  The runtime spreads a process's streams over a few hardware queues (four by
    default), and a stream that shares its queue with the null stream holds null-stream work back behind its own:
    on such a stream a launch on the wrong stream would go unseen.  In a process that has made many streams before
    (the whole suite in one go) the next new stream can be such a one, so: the first of up to eight new streams whose
    pending delay the default stream overtakes.  Should none do, the last is returned and control 1 says so."""
    s = None
    for k in range(8):
        s = torch.cuda.Stream()
        if _overtakes(s, cycles_per_ms * 10):
            print(f"[streams] side stream: candidate {k}")
            break
    return s


@pytest.fixture(scope="module")
def delay_cycles(be, side, cycles_per_ms):
    """Cycles for a delay of at least ``DELAY_MS`` on ``s``, checked with an event pair on ``s``."""
    assert 20.0 <= DELAY_MS <= DELAY_CAP_MS
    cycles = int(cycles_per_ms * DELAY_MS * 1.25)
    held = _timed_sleep(side, cycles)
    print(f"[streams] _sleep: {cycles_per_ms:,.0f} cycles per ms; {cycles:,} cycles hold the stream for {held:.1f} ms")
    assert DELAY_MS <= held <= DELAY_CAP_MS, (cycles_per_ms, cycles, held)
    return cycles


@gpu
def test_control_null_stream_work_overtakes_the_side_stream(be, side, delay_cycles):
    """Control 1: behind the delay and the FRESH copies on ``s``, a clone issued under the default stream still reads
    STALE and one issued under ``s`` reads FRESH."""
    c = H.CASES["count_overlaps"]
    early, late = H.control_clones(be, side, c.inputs("stale"), c.inputs("fresh"), delay_cycles)
    for k, v in c.inputs("stale").items():
        assert H.bitwise_equal(early[k], v), f"{k}: default-stream work waited for the side stream"
    for k, v in c.inputs("fresh").items():
        assert H.bitwise_equal(late[k], v), k


@gpu
def test_control_a_mis_streamed_entry_point_answers_from_stale_rows(be, side, delay_cycles, engines, monkeypatch):
    """Control 2: ``count_overlaps`` with ``HipEngine._stream`` returning the null stream.  The kernels then run
    before the delay ends, on STALE rows -- exactly what an entry point that ignores its stream argument does -- and
    the protocol shows it.

    With nothing but ``_stream`` patched the counts come back all zero (measured on an MI355X): the engine's own
    ``torch.zeros`` of the counts stays on ``s``, behind the delay, and wipes what the early kernels wrote.  That is
    neither answer, so the control runs twice: as it is -- the result must not be ``reference(FRESH)`` -- and with
    counts that were zeroed before step 1 handed to the engine, where it must be ``reference(STALE)``.

    The context is the one that never forks its second stream.  On the default context ``SideChain`` sorts the
    query side on the context's own stream, and when that stream shares its hardware queue with ``s`` it waits
    behind the delay and reads FRESH rows while the rest reads STALE ones: a mix (observed), still not FRESH, but
    nothing to compare with."""
    from giql_amd.engine import HipEngine

    c, eng = H.CASES["count_overlaps"], engines["local"]
    stale, fresh = c.inputs("stale"), c.inputs("fresh")
    n_a = fresh["a.chrom"].shape[0]
    real_stream, real_zeros = HipEngine._stream, torch.zeros
    monkeypatch.setattr(HipEngine, "_stream", lambda self: ctypes.c_void_p(0))
    try:
        wiped, _ = H.run_protocol(be, side, stale, fresh, lambda bufs: c.run(eng, bufs, None), delay_cycles)
        counts = real_zeros(n_a, dtype=torch.int64, device=eng.device)
        monkeypatch.setattr(torch, "zeros", lambda *a, **kw: counts if a == (n_a,) and kw.get("dtype") == torch.int64
                            else real_zeros(*a, **kw))
        out, clones = H.run_protocol(be, side, stale, fresh, lambda bufs: c.run(eng, bufs, None), delay_cycles)
    finally:
        monkeypatch.undo()
    assert HipEngine._stream is real_stream and torch.zeros is real_zeros
    assert not H.same(wiped, c.want("fresh")), "a call on the null stream went unnoticed"
    assert H.same(out, c.want("stale")), "the null-stream call did not overtake the pending copies"
    assert not H.same(out, c.want("fresh"))
    for k, v in fresh.items():
        assert H.bitwise_equal(clones[k], v), k


#: cases whose last sort tells, in the context's statistics, whether ``SideChain`` could fork
FORKS = {"inner_join[general]": False, "semi_join": False, "count_overlaps": False,
         "inner_join[general]@local": True, "semi_join@local": True, "count_overlaps@local": True}


@gpu
@pytest.mark.parametrize("cid", list(H.CASES))
def test_on_a_side_stream_behind_pending_work(cid, be, side, delay_cycles, engines):
    c = H.CASES[cid]
    eng = engines[c.engine]
    prepared = c.prepare(eng) if c.prepare else None
    stale, fresh, want = c.inputs("stale"), c.inputs("fresh"), c.want("fresh")
    for rnd in (1, 2):      # the second run starts from the guesses the first left on the context
        out, clones = H.run_protocol(be, side, stale, fresh, lambda bufs: c.run(eng, bufs, prepared), delay_cycles)
        got = c.canon(out, fresh) if c.canon else out
        assert H.same(got, want), (cid, rnd, "the result is not reference(FRESH)")
        for k, v in fresh.items():
            assert k in c.exempt or H.bitwise_equal(clones[k], v), (cid, rnd, k, "an input was written")
        if cid in FORKS:
            assert eng.stats()["sort_local"] == FORKS[cid], (cid, rnd)
    del prepared


# ---- execute(): host Arrow tables in, one table out; under ``s`` behind a delay it returns what it returns on the
# default stream
def _pa_rows(tbl):
    return sorted(zip(*(tbl.column(n).to_pylist() for n in tbl.column_names)), key=repr)


def _execute_cases():
    import json
    import os

    import _left_ref as L
    from giql_amd.execute import execute
    from giql_amd.table import Table
    from giql_amd.transpile import transpile

    pa = pytest.importorskip("pyarrow")
    here = os.path.dirname(os.path.abspath(__file__))
    golden = lambda name: json.load(open(os.path.join(here, "golden", name)))
    pg = L.make_tables()
    on = "ON a.interval INTERSECTS b.interval"
    plan = lambda q: transpile(q, tables=["peaks", "genes"], dialect="hip")
    cases = {
        "INNER": lambda eng: execute(plan(f"SELECT a.name AS a_name, a.start AS a_start, b.name AS b_name, b.end AS b_end "
                                          f"FROM peaks a JOIN genes b {on}"), pg, eng),
        "SEMI": lambda eng: execute(plan(f"SELECT a.chrom, a.start, a.end FROM peaks a SEMI JOIN genes b {on}"), pg, eng),
        "NEAREST k=2": lambda eng: execute(plan(
            "SELECT a.start AS a_start, b.start AS b_start, b.distance AS d FROM peaks a "
            "CROSS JOIN LATERAL NEAREST(genes, reference := a.interval, k := 2) b"), pg, eng),
    }
    ma = golden("merge_aggregates.json")
    types = [pa.string(), pa.int32(), pa.int32(), pa.string(), pa.float64(), pa.int32()]
    features = pa.table({c: pa.array([r[k] for r in ma["rows"]], type=t) for k, (c, t) in enumerate(zip(ma["columns"], types))})
    cases["MERGE with aggregates"] = lambda eng: execute(
        "SELECT MERGE(interval, 1000), COUNT(*) AS n, AVG(score) AS avg_score, MAX(score) AS hi FROM features",
        {"features": features}, eng, giql_tables=["features"], merge_aggregates=True)
    dj = max((c for c in golden("disjoin.json")["cases"] if c["reference"] is not None and tuple(c["encoding"]) ==
              ("0based", "half_open")), key=lambda c: len(c["expected"]))
    from test_disjoin_gpu import _table as dj_table
    cases["DISJOIN"] = lambda eng: execute(
        transpile("SELECT * FROM DISJOIN(features, reference := refs)", [Table("features"), "refs"], dialect="hip"),
        {"features": dj_table(dj["target"]), "refs": dj_table(dj["reference"])}, eng)
    from test_range_sets_gpu import _arrow_table, _giql_tables
    rs = max((c for c in golden("range_sets.json")["cases"] if " ANY(" in c["where"]), key=lambda c: len(c["expected"]))
    cases["range set"] = lambda eng: pa.table({"row": execute(
        "SELECT * FROM t WHERE " + rs["where"], {"t": _arrow_table(rs)}, eng, giql_tables=_giql_tables(rs),
        return_indices=True, range_sets=True)})
    # the three opt-ins that end in the pair aggregates and in coverage: a query of each fixed list, on the tables of
    # tests/test_join_aggregates_gpu.py (300 x 700 rows; the coverage recipe reads the left one)
    import _agg_expr_queries as XQ
    import _coverage_queries as CQ
    import _join_agg_queries as JQ
    import test_join_aggregates_gpu as JA

    r = np.random.default_rng(2026)
    ab = {"a": JA._arrow(JA._table(r, 300, ["g1", "g2", "g3", "g4", "g5", "g6", "g7"])),
          "b": JA._arrow(JA._table(r, 700, ["x", "y", "z"]))}
    cases["join aggregates"] = lambda eng: execute(JQ.MAP_SHAPE["eight_aggregates"], ab, eng, giql_tables=JQ.TABLES,
                                                   join_aggregates=True)
    cases["aggregate expressions"] = lambda eng: execute(XQ.IN_SHAPE["weighted"], ab, eng, giql_tables=XQ.TABLES,
                                                         join_aggregates=True, aggregate_expressions=True)
    cases["coverage"] = lambda eng: execute(CQ.DEPTH, {"features": ab["a"]}, eng, giql_tables=CQ.TABLES,
                                            disjoin_aggregates=True)
    return cases


EXECUTE_QUERIES = ["INNER", "SEMI", "NEAREST k=2", "MERGE with aggregates", "DISJOIN", "range set", "join aggregates",
                   "aggregate expressions", "coverage"]


def test_the_execute_queries_have_a_case_each_and_lower_under_their_opt_in():
    """CPU: the three queries added for the pair aggregates and coverage are inside the shape their opt-in lowers --
    the plan says so -- so the GPU test below reaches ``pair_agg``, ``pair_expr_agg`` and ``coverage`` and not an
    older route."""
    import _agg_expr_queries as XQ
    import _coverage_queries as CQ
    import _join_agg_queries as JQ
    from giql_amd.transpile import build_plan

    assert set(EXECUTE_QUERIES) >= {"join aggregates", "aggregate expressions", "coverage"}
    plan = build_plan(JQ.MAP_SHAPE["eight_aggregates"], JQ.TABLES, join_aggregates=True)
    assert plan.join_aggregates and len(plan.aggregates) == 8 and not plan.expressions, plan.to_string()
    plan = build_plan(XQ.IN_SHAPE["weighted"], XQ.TABLES, join_aggregates=True, aggregate_expressions=True)
    assert plan.join_aggregates and len(plan.expressions) == 1, plan.to_string()
    assert [(a.func, a.side) for a in plan.aggregates] == [("SUM", "x"), ("AVG", "r")]      # a tree beside a plain column
    assert CQ.ACCEPTED["depth_recipe"] == (CQ.DEPTH, "depth")
    assert build_plan(CQ.DEPTH, CQ.TABLES, disjoin_aggregates=True).segments == "depth"


@gpu
@pytest.mark.parametrize("name", EXECUTE_QUERIES)
def test_execute_on_a_side_stream_returns_the_default_streams_table(name, be, side, delay_cycles, engines):
    run = _execute_cases()[name]
    eng = engines["default"]
    want = run(eng)
    torch.cuda.synchronize()
    assert want.num_rows > 0
    for _rnd in (1, 2):
        with torch.cuda.stream(side):
            torch.cuda._sleep(delay_cycles)
            got = run(eng)
        side.synchronize()
        assert got.schema == want.schema and _pa_rows(got) == _pa_rows(want), name
