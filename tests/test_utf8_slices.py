"""The row split of a string projection past int32 offsets (``execute.plan_utf8_slices``): pure numpy, no GPU.

One ``giql_hip_take_utf8_*`` call gathers at most 0x7FFFFFFF bytes and 0x7FFFFFF0 rows; ``execute`` splits a larger
gather into consecutive row slices, each as long as the limits allow, and returns the column in that many chunks."""

import numpy as np
import pytest

from giql_amd.execute import UTF8_MAX_BYTES, UTF8_MAX_ROWS, plan_utf8_slices


def _check(lengths, slices, max_bytes, max_rows):
    """Consecutive, non-empty, covering, within both limits, and greedy: no slice could take its successor's first row."""
    lengths = np.asarray(lengths, np.int64)
    assert [lo for lo, _ in slices] == [0] + [hi for _, hi in slices[:-1]]
    assert (slices[-1][1] if slices else 0) == lengths.shape[0]
    for k, (lo, hi) in enumerate(slices):
        assert hi > lo and hi - lo <= max_rows and int(lengths[lo:hi].sum()) <= max_bytes
        if k + 1 < len(slices):
            assert hi - lo == max_rows or int(lengths[lo:hi + 1].sum()) > max_bytes


def test_limits_match_the_c_abi():
    assert (UTF8_MAX_BYTES, UTF8_MAX_ROWS) == (0x7FFFFFFF, 0x7FFFFFF0)


def test_empty_input_has_no_slice():
    assert plan_utf8_slices(np.zeros(0, np.int32)) == []
    assert plan_utf8_slices(np.zeros(0, np.int32), 10, 3) == []


def test_a_fitting_column_is_one_slice():
    lengths = np.array([5, 0, 17, 3], np.int32)
    assert plan_utf8_slices(lengths) == [(0, 4)]
    assert plan_utf8_slices(np.zeros(1000, np.int32), 1, 1000) == [(0, 1000)]   # empty strings cost no byte


def test_total_exactly_at_the_limit_is_one_slice():
    assert plan_utf8_slices(np.array([4, 3, 3], np.int32), 10, 100) == [(0, 3)]
    # at the real limit: 32767 rows of 65536 bytes plus one remainder row make 2^31 - 1 bytes
    lengths = np.full(32768, 65536, np.int32)
    lengths[-1] = 65535
    assert int(lengths.astype(np.int64).sum()) == 2**31 - 1
    assert plan_utf8_slices(lengths) == [(0, 32768)]


def test_one_byte_over_the_limit_splits_before_the_last_row():
    assert plan_utf8_slices(np.array([4, 3, 4], np.int32), 10, 100) == [(0, 2), (2, 3)]
    lengths = np.full(32768, 65536, np.int32)     # 2^31 bytes: one more than an int32 offset holds
    assert plan_utf8_slices(lengths) == [(0, 32767), (32767, 32768)]


def test_a_row_longer_than_the_limit_is_refused():
    with pytest.raises(ValueError, match="row 2 is 11 bytes"):
        plan_utf8_slices(np.array([1, 2, 11, 1], np.int32), 10, 100)
    with pytest.raises(ValueError, match="negative"):
        plan_utf8_slices(np.array([1, -1], np.int32), 10, 100)


def test_limits_on_rows_only():
    assert plan_utf8_slices(np.zeros(7, np.int32), 10, 3) == [(0, 3), (3, 6), (6, 7)]
    assert plan_utf8_slices(np.ones(6, np.int32), 100, 2) == [(0, 2), (2, 4), (4, 6)]


@pytest.mark.parametrize("seed", range(6))
def test_random_lengths_against_the_definition(seed):
    r = np.random.default_rng(seed)
    lengths = r.integers(0, 40, int(r.integers(1, 3000))).astype(np.int32)
    lengths[r.random(lengths.shape[0]) < 0.3] = 0
    max_bytes = int(r.integers(40, 2000))
    max_rows = int(r.integers(1, 400))
    slices = plan_utf8_slices(lengths, max_bytes, max_rows)
    _check(lengths, slices, max_bytes, max_rows)
    # the same split, one row at a time
    want, lo, acc = [], 0, 0
    for i, ln in enumerate(lengths.tolist()):
        if i > lo and (acc + ln > max_bytes or i - lo == max_rows):
            want.append((lo, i))
            lo, acc = i, 0
        acc += ln
    want.append((lo, lengths.shape[0]))
    assert slices == want


def test_int32_lengths_do_not_overflow_the_running_total():
    lengths = np.full(5, 2**31 - 1, np.int32)     # each row alone is at the limit
    assert plan_utf8_slices(lengths) == [(k, k + 1) for k in range(5)]
