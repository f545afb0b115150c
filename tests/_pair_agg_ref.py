"""Aggregates over a join's pairs per left row, restated with numpy and plain Python: the pairs are ordered by
(row_a, row_b) -- a row's values are reduced in ascending ``row_b`` -- and every aggregate is computed exactly:
Python ``int`` sums, ``math.fsum`` for float sums, ``float(sum) / count`` for AVG.  NULLs (``None``) are skipped, a
row without a non-NULL input yields ``None`` (COUNT: 0).  NaN follows DuckDB's total order, in which NaN is greater
than every number: MAX of a group with a NaN is NaN, MIN ignores NaNs unless every non-NULL value is one, SUM
propagates.  The result is a function of the SET of pairs."""
import math

import numpy as np


def _is_nan(v) -> bool:
    return isinstance(v, float) and v != v


def aggregate(func: str, values):
    """One aggregate over a group's values (``None`` = NULL), exact."""
    vals = [v for v in values if v is not None]
    if func == "COUNT":
        return len(vals)
    if not vals:
        return None
    flt = any(isinstance(v, float) for v in vals)
    if func in ("SUM", "AVG"):
        total = math.fsum(v for v in vals if not _is_nan(v) and not math.isinf(v)) if flt else sum(vals)
        if flt:
            infs = {v for v in vals if math.isinf(v)}
            if any(_is_nan(v) for v in vals) or len(infs) == 2:
                total = float("nan")
            elif infs:
                total = infs.pop()
        return total if func == "SUM" else float(total) / len(vals)
    numbers = [v for v in vals if not _is_nan(v)]
    if func == "MIN":
        return min(numbers) if numbers else float("nan")
    if func == "MAX":
        return max(numbers) if len(numbers) == len(vals) else float("nan")
    raise ValueError(func)


def members(row_a, row_b, n_a: int):
    """Per A row the B rows of its pairs, ascending (duplicates kept)."""
    row_a, row_b = np.asarray(row_a, np.int64), np.asarray(row_b, np.int64)
    order = np.lexsort((row_b, row_a))
    out = [[] for _ in range(n_a)]
    for a, b in zip(row_a[order].tolist(), row_b[order].tolist()):
        out[a].append(b)
    return out


def pair_aggregate(row_a, row_b, n_a: int, columns, aggs):
    """``(pairs, results)``: ``pairs[a]`` the pairs of A row ``a``; ``results[j][a]`` the value of ``aggs[j]`` for
    it (``None`` = NULL).  ``columns``: name -> per-B-row Python values (``None`` = NULL); ``aggs``: ``[(func, column
    name)]``."""
    mem = members(row_a, row_b, n_a)
    return ([len(m) for m in mem],
            [[aggregate(f, [columns[c][b] for b in m]) for m in mem] for f, c in aggs])


def abs_sum(values) -> float:
    """Sum of |x| over the non-NULL, finite values: the scale of a float sum's error bound."""
    return math.fsum(abs(v) for v in values if v is not None and not _is_nan(v) and not math.isinf(v))
