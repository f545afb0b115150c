"""The sort scratch a call zeroes up front, on a workspace that is anything but zero.

A call that sorts zeroes its digit histograms and onesweep status words with one memset up front and records the range
in the context's ledger (``giql_amd/csrc/zero_ledger.h``); the helpers skip their own memsets for the buffers the
ledger hands them.  A status word that is wrongly taken for zero does not give a wrong number, it sends the look-back
after a tile that never ran -- so every case here first runs a DISJOIN over 20,000 rows, which leaves the workspace
full of its own arrays, and then the calls in which a buffer is used a second time or lies outside the first memset:

* (a) NEAREST: the one-sort plan, then a table with pile-ups -- the two-sort plan sorts B twice through one set of
  status words;
* (b) COUNT: a fixed-length B, then a variable-length one -- the general form sorts B's starts and ends through one
  set of status words;
* (c) INNER plan: the fixed-length form, then the general one -- the layout guess misses, and a side whose histogram
  the span pass counted into is linearized after all;
* (d) INNER plans at densities on either side of a bucket-width change (16-bit buckets: two global passes, narrower
  ones: three, none: four) -- the larger side needs more zeroed passes than the first memset gave it;
* (e) index create, then the indexed join, on a fixed-length table of 30,000 rows;
* (f) coverage, then an INNER plan of the general form -- coverage's event sort and its three scans carve status words
  and histograms where the plan's two sides then carve theirs;
* (g) an INNER plan over a fixed-length B (its span pass counts into the histogram), then coverage of that B;
* (h) a pair aggregate (two radix sorts and a scan of its own carve), then NEAREST on pile-ups: the two-sort plan;
* (i) NEAREST, then both pair aggregates, then coverage;
* (j) coverage runs, DISJOIN of the same table, coverage depth: the two entry points share the front's carves.

One context with the production density rules and no row floor; each call runs twice (on the previous call's guesses,
then on its own) and is checked against the C oracle.  The classes, their resident copies and their cached oracle
answers are those of ``tests/test_context_transitions.py``.
"""

import numpy as np
import pytest

from oracle import pyoracle as ora

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import test_context_transitions as tr

    with pytest.MonkeyPatch.context() as mp:
        e = tr._density_engine(mp)
    yield e
    e.close()


def _dirty(eng):
    """A DISJOIN over the 20,000 rows of ``general``'s B: its events, breakpoints and offsets now lie where the next
    call carves its histograms and status words."""
    import test_context_transitions as tr

    _a, b, nch, _da, db = tr.resident("general")
    parent, _ds, _de = eng.disjoin(db, None, nch)
    assert b.n == 20_000 and int(parent.shape[0]) >= b.n


def _twice(eng, op, names, fam):
    import test_context_transitions as tr

    log = tr.Log()
    _dirty(eng)
    for name in names:
        for rnd in (1, 2):
            op(eng, name, log, fam, rnd)
    return log


def test_nearest_one_sort_then_two_sorts(eng):
    import test_context_transitions as tr

    _twice(eng, tr.op_nearest, ["general", "pileups", "general"], "nearest")


def test_count_fixed_length_then_general(eng):
    import test_context_transitions as tr

    log = _twice(eng, tr.op_count, ["uniform_b", "general", "uniform_b"], "row")
    forms = [c[4]["join_form"] for c in log.calls if c[2] == 2]
    assert forms == ["uniform_b", "general", "uniform_b"], forms    # (bit 0 of the form word: B was fixed-length)


def test_inner_plan_fixed_length_then_general(eng):
    import test_context_transitions as tr

    log = _twice(eng, tr.op_plan_fill, ["uniform_b", "general", "uniform_b"], "inner")
    forms = [c[4]["join_form"] for c in log.calls if c[2] == 2]
    assert forms == ["uniform_b", "general", "uniform_b"], forms


@pytest.fixture(scope="module")
def wide_general():
    """100,000 variable-length rows over four chromosomes: as many rows as ``w16``, on an axis several times as long."""
    import test_context_transitions as tr

    r = np.random.default_rng(3140)
    a, b = tr._rows(r, 3000, 4, 8_000_000, (1, 2000)), tr._rows(r, 100_000, 4, 8_000_000, (1, 800))
    return tr._dev(a), tr._dev(b), 4, ora.sort_pairs(*ora.c_inner(a, b, "sweep"))


def _plan_fill(eng, da, db, nch, want):
    import test_context_transitions as tr

    n = eng.inner_plan(da, db, nch)
    st = eng.stats()
    assert n == want.shape[0]
    ra = torch.empty(n, dtype=torch.int32, device="cuda:0")
    rb = torch.empty(n, dtype=torch.int32, device="cuda:0")
    eng.inner_fill(ra, rb)
    assert np.array_equal(tr._pairs(ra, rb), want)
    return st


def test_inner_plans_across_a_bucket_width_change(eng, wide_general):
    """``w16`` settles on 16-bit buckets: two global passes.  The next plan has as many rows and another form, so it is
    repeated without speculation on ``w16``'s density -- two passes of the larger side's status words are zeroed up
    front -- and reads back a density that takes no buckets at all: four passes.  Then the way back."""
    import test_context_transitions as tr

    _a, _b, nch16, da16, db16 = tr.resident("w16")
    _dirty(eng)
    for _leg in (1, 2):
        for _rnd in (1, 2):
            st = _plan_fill(eng, da16, db16, nch16, tr.want("w16", "pairs"))
        assert st["join_form"] == "uniform_b" and st["sort_local"] and st["bucket_bits"] == 16, st
        for _rnd in (1, 2):
            st = _plan_fill(eng, *wide_general)
            assert st["join_form"] == "general" and not st["sort_local"], st


@pytest.fixture(scope="module")
def fixed_30k():
    import test_context_transitions as tr

    r = np.random.default_rng(3130)
    a, b = tr._rows(r, 3000, 4, 8_000_000, (1, 2000)), tr._rows(r, 30_000, 4, 8_000_000, 150)
    return tr._dev(a), tr._dev(b), 4, ora.sort_pairs(*ora.c_inner(a, b, "sweep"))


def test_index_create_then_indexed_join(eng, fixed_30k):
    import test_context_transitions as tr

    da, db, nch, want = fixed_30k
    assert want.shape[0] > 0
    _dirty(eng)
    for _rnd in (1, 2):
        index = eng.index_create(db, nch)
        try:
            ra, rb = eng.inner_join_indexed(da, index)
            assert np.array_equal(tr._pairs(ra, rb), want)
        finally:
            index.close()


def _in_turn(eng, steps, fam):
    """``steps`` = ``[(operator, class)]``, the whole sequence twice on the dirtied workspace: every call runs right
    after the one before it in the list, first on that call's leavings alone and then on its own as well."""
    import test_context_transitions as tr

    log = tr.Log()
    _dirty(eng)
    for rnd in (1, 2):
        for op, name in steps:
            op(eng, name, log, fam, rnd)
    return log


def test_coverage_then_inner_plan(eng):
    import test_context_transitions as tr

    log = _in_turn(eng, [(tr.op_coverage, "general"), (tr.op_plan_fill, "general")], "mixed")
    assert [c[3] for c in log.calls] == ["coverage", "plan"] * 2
    assert log.calls[-1][4]["join_form"] == "general"


def test_inner_plan_over_a_fixed_length_b_then_coverage(eng):
    import test_context_transitions as tr

    log = _in_turn(eng, [(tr.op_plan_fill, "uniform_b"), (tr.op_coverage, "uniform_b")], "mixed")
    plans = [c[4] for c in log.calls if c[3] == "plan"]
    assert plans[-1]["join_form"] == "uniform_b", plans[-1]["join_form"]


def test_pair_aggregate_then_nearest_with_two_sorts(eng):
    import test_context_transitions as tr

    _in_turn(eng, [(tr.op_pair_agg, "pileups"), (tr.op_nearest, "pileups")], "mixed")


def test_nearest_then_pair_aggregates_then_coverage(eng):
    import test_context_transitions as tr

    _in_turn(eng, [(tr.op_nearest, "general"), (tr.op_pair_agg, "general"), (tr.op_pair_expr_agg, "general"),
                   (tr.op_coverage, "general")], "mixed")


def test_coverage_runs_then_disjoin_then_coverage_depth(eng):
    """One table through the three calls that carve DISJOIN's front: spans, 2n events, one sort, two flag scans."""
    import test_context_transitions as tr
    from _disjoin_ref import brute_force_arrays

    _a, b, nch, _da, db = tr.resident("general")
    pieces = brute_force_arrays(b.chrom.astype(np.int64), b.start.astype(np.int64), b.end.astype(np.int64))
    same = lambda out, want: all(g.shape == w.shape and torch.equal(g, w) for g, w in zip(out, want))  # noqa: E731
    _dirty(eng)
    for _rnd in (1, 2):
        assert same(eng.coverage(db, nch, runs=True), tr.want_coverage("general", True)), "coverage runs"
        got = tr._pieces(*eng.disjoin(db, None, nch))
        assert got.shape == pieces.shape and np.array_equal(got, pieces), "disjoin"
        assert same(eng.coverage(db, nch), tr.want_coverage("general", False)), "coverage depth"
