"""Per-left-row reductions of a pair list: what SEMI, ANTI and COUNT over a pair predicate must equal.

``pairs`` is any ``[[row_a, row_b], ...]`` (a fixture's list, a brute force's array, a pair join's output); numpy
only."""

import numpy as np


def reduce_pairs(pairs, n_a: int):
    """``(semi ids, anti ids, counts)`` of ``n_a`` left rows: the ascending ids of the rows with / without a pair
    and one int64 count per row."""
    p = np.asarray(pairs, np.int64).reshape(-1, 2)
    counts = np.bincount(p[:, 0], minlength=int(n_a)).astype(np.int64)
    assert counts.size == int(n_a), "a pair names a left row past the table"
    ids = np.arange(int(n_a), dtype=np.int64)
    return ids[counts > 0], ids[counts == 0], counts


def transpose(pairs):
    """The pairs with their columns exchanged (``b <predicate'> a`` from ``a <predicate> b``)."""
    return np.asarray(pairs, np.int64).reshape(-1, 2)[:, ::-1]


def window_counts(ac, as_, ae, bc, bs, be, n: int, chunk: int = 1 << 22):
    """int64 counts per A row of the B rows on its chromosome with ``a.start - n < b.end AND a.end + n > b.start``
    (canonical coordinates, start <= end on every row: there it is DISTANCE(a, b) <= n).  A chunked brute force over
    the boolean matrix, for tables ``_distance_ref.window_pairs`` would not hold."""
    ac, as_, ae, bc, bs, be = (np.asarray(x, np.int64) for x in (ac, as_, ae, bc, bs, be))
    out = np.zeros(ac.size, np.int64)
    if bc.size == 0:
        return out
    step = max(1, chunk // bc.size)
    for lo in range(0, ac.size, step):
        hi = min(ac.size, lo + step)
        m = ((ac[lo:hi, None] == bc[None, :]) & (as_[lo:hi, None] - n < be[None, :]) & (ae[lo:hi, None] + n > bs[None, :]))
        out[lo:hi] = m.sum(1)
    return out
