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
* (e) index create, then the indexed join, on a fixed-length table of 30,000 rows.

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
