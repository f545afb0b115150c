"""MERGE with aggregates restated in plain Python: the reference keeps a plain aggregate beside MERGE and evaluates
it under the per-cluster GROUP BY (src/giql/expanders/merge.py:317-390).  Cluster ids come from the oracle
(``c_cluster``, or ``py_cluster_predicate`` for the ``predicate :=`` form); rows are grouped by (partition, id) and
every aggregate is computed exactly: Python ``int`` sums, ``math.fsum`` for float sums, ``float(sum) / count`` for
AVG.  NULLs (``None``) are skipped, a group without a non-NULL input yields ``None`` (COUNT: 0).  NaN follows
DuckDB's total order, in which NaN is greater than every number: MAX of a group with a NaN is NaN, MIN ignores NaNs
unless every non-NULL value is one, SUM propagates."""
import math

import numpy as np

from oracle import pyoracle as ora


def cluster_ids(part, start, end, distance=0, holds=None):
    """Cluster id per row, 1-based inside its partition (``part``: any sortable, hashable value per row)."""
    if holds is not None:
        return ora.py_cluster_predicate(list(part), list(start), list(end), distance, holds).tolist()
    codes = {p: k for k, p in enumerate(sorted(set(part)))}
    side = ora.Side(np.array([codes[p] for p in part], np.int32), np.asarray(start), np.asarray(end))
    # (the C restatement: py_cluster, the same window SQL in plain Python, is quadratic -- tests/test_merge_aggregates.py
    # holds the two to each other on the golden rows)
    return ora.c_cluster(side, distance).tolist()


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
        total = math.fsum(vals) if flt else sum(vals)
        if flt and any(_is_nan(v) for v in vals):
            total = float("nan")
        return total if func == "SUM" else float(total) / len(vals)
    numbers = [v for v in vals if not _is_nan(v)]
    if func == "MIN":
        return min(numbers) if numbers else float("nan")
    if func == "MAX":
        return max(numbers) if len(numbers) == len(vals) else float("nan")
    raise ValueError(func)


def regions(part, start, end, distance=0, holds=None):
    """``[(partition, [row, ...])]`` of the merged regions, ordered by (partition, MIN(start))."""
    ids = cluster_ids(part, start, end, distance, holds)
    groups: dict = {}
    for i, key in enumerate(zip(part, ids)):
        groups.setdefault(key, []).append(i)
    return sorted(((p, members) for (p, _cid), members in groups.items()),
                  key=lambda g: (g[0], min(int(start[i]) for i in g[1])))


def merge_agg(part, start, end, distance, columns, aggs, holds=None):
    """Rows ``[partition, MIN(start), MAX(end), COUNT(*), aggregate, ...]`` ordered by (partition, start).
    ``columns``: name -> per-row values; ``aggs``: ``[(func, column name)]``."""
    return [[p, min(int(start[i]) for i in members), max(int(end[i]) for i in members), len(members)]
            + [aggregate(f, [columns[c][i] for i in members]) for f, c in aggs]
            for p, members in regions(part, start, end, distance, holds)]


def abs_sum(values) -> float:
    """Sum of |x| over the non-NULL, finite values: the scale of a float sum's error bound."""
    return math.fsum(abs(v) for v in values if v is not None and not _is_nan(v) and not math.isinf(v))
