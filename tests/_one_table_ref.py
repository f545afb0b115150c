"""CLUSTER, MERGE and MERGE's aggregates restated in numpy: the semantics of ``oracle.pyoracle.py_cluster`` /
``py_merge``, ``tests/_merge_agg_ref.py`` and ``tests/_string_agg_ref.py`` for tables of a few 100,000 rows, where the
row-by-row restatements take minutes.  ``tests/test_one_table_ref.py`` holds this file to those four on seeded tables.

Rows are ordered by (chrom, start, input row).  Inside a chromosome a row is a region head when it is the first row or
when ``start > running MAX(end) of the rows before it + distance``.  Integers are int64 throughout (``Layout.int_sum``
asserts that no sum can reach 2^63); a float SUM is ``math.fsum`` in binary64 -- correctly rounded, so more precise than
any summation order a kernel may take; NULL and NaN follow DuckDB as ``_merge_agg_ref.aggregate`` states it.  The
``predicate :=`` form stays with the row-by-row references."""
import math

import numpy as np

I64_MAX = np.iinfo(np.int64).max
I64_MIN = np.iinfo(np.int64).min


class Layout:
    """The sorted order and the regions of one table at one ``distance``."""

    def __init__(self, chrom, start, end, distance=0):
        chrom, start, end = (np.asarray(x).astype(np.int64) for x in (chrom, start, end))
        n = self.n = int(chrom.shape[0])
        self.order = order = np.lexsort((np.arange(n), start, chrom))
        c, s, e = chrom[order], start[order], end[order]
        self.first = first = np.ones(n, bool)
        first[1:] = c[1:] != c[:-1]
        # running MAX(end) inside a chromosome: chromosome k's ends lifted to [k * big, (k + 1) * big), so that the
        # running maximum over the whole order never carries a value across a chromosome's first row
        lo = int(e.min()) if n else 0
        big = (int(e.max()) - lo + 1) if n else 1
        block = np.cumsum(first) - 1
        run = np.maximum.accumulate(block * big + (e - lo)) - block * big + lo
        before = np.empty(n, np.int64)
        before[1:] = run[:-1]
        self.head = head = first.copy()
        head[1:] |= s[1:] > before[1:] + max(int(distance), 0)
        self.heads = heads = np.nonzero(head)[0]
        self.m = int(heads.shape[0])
        self.region = np.cumsum(head) - 1                       # region of a sorted position
        self.count = np.diff(np.append(heads, n)).astype(np.int64)
        self.c, self.s, self.e = c, s, e

    # ---- CLUSTER / MERGE
    def cluster_ids(self):
        """Per input row, 1-based inside its chromosome: ``ora.c_cluster``."""
        rank = np.cumsum(self.head)
        first_pos = np.maximum.accumulate(np.where(self.first, np.arange(self.n), 0))
        ids = np.empty(self.n, np.int64)
        ids[self.order] = rank - rank[first_pos] + 1 if self.n else rank
        return ids

    def merge_rows(self):
        """``(chrom, start, end, count)`` per region, ordered by (chrom, start): ``ora.c_merge``."""
        if self.n == 0:
            z = np.zeros(0, np.int64)
            return z, z, z, z
        return self.c[self.heads], self.s[self.heads], np.maximum.reduceat(self.e, self.heads), self.count

    # ---- numeric aggregates: ``(values, valid)`` per region
    def _sorted(self, values, valid):
        v = np.asarray(values)[self.order]
        ok = np.ones(self.n, bool) if valid is None else np.asarray(valid).astype(bool)[self.order]
        return v, ok

    def non_null(self, valid):
        """COUNT(column) per region."""
        ok = np.ones(self.n, bool) if valid is None else np.asarray(valid).astype(bool)[self.order]
        return np.add.reduceat(ok.astype(np.int64), self.heads) if self.n else np.zeros(0, np.int64)

    def int_sum(self, values, valid):
        v, ok = self._sorted(values, valid)
        v = np.where(ok, v.astype(np.int64), 0)
        assert sum(abs(int(x)) for x in v[v != 0].tolist()) < 2**63, "an integer sum could reach 2^63"
        return np.add.reduceat(v, self.heads)

    def float_sum(self, values, valid):
        """``math.fsum`` of the non-NULL values per region; NaN where one of them is NaN."""
        v, ok = self._sorted(values, valid)
        v = v.astype(np.float64)
        nan = np.add.reduceat((ok & np.isnan(v)).astype(np.int64), self.heads) > 0
        x = np.where(ok & ~np.isnan(v), v, 0.0).tolist()         # (a zero adds nothing to an exact sum)
        bounds = np.append(self.heads, self.n).tolist()
        out = np.array([math.fsum(x[a:b]) for a, b in zip(bounds, bounds[1:])], np.float64)
        out[nan] = np.nan
        return out

    def abs_sum(self, values, valid):
        """``fsum`` of |x| over the non-NULL finite values per region: the scale of a float sum's error bound."""
        v, ok = self._sorted(values, valid)
        v = v.astype(np.float64)
        x = np.where(ok & np.isfinite(v), np.abs(v), 0.0).tolist()
        bounds = np.append(self.heads, self.n).tolist()
        return np.array([math.fsum(x[a:b]) for a, b in zip(bounds, bounds[1:])], np.float64)

    def aggregate(self, func, values, valid=None):
        """One aggregate over every region: ``(values, valid)``.  COUNT and the SUM / MIN / MAX of an integer column
        are int64, everything over a float column and every AVG float64; a value where ``valid`` is false is 0."""
        func = func.upper()
        k = self.non_null(valid)
        if func == "COUNT":
            return k, np.ones(self.m, bool)
        some = k > 0
        flt = np.asarray(values).dtype.kind == "f"
        v, ok = self._sorted(values, valid)
        if func in ("SUM", "AVG"):
            total = self.float_sum(values, valid) if flt else self.int_sum(values, valid)
            if func == "AVG":
                total = total.astype(np.float64) / np.where(some, k, 1)
        elif not flt:
            fill, red = (I64_MAX, np.minimum) if func == "MIN" else (I64_MIN, np.maximum)
            total = red.reduceat(np.where(ok, v.astype(np.int64), fill), self.heads)
        elif func == "MIN":       # NaN is greater than every number: ignored unless every non-NULL value is one
            total = np.fmin.reduceat(np.where(ok, v.astype(np.float64), np.nan), self.heads)
        elif func == "MAX":       # ... and wins whenever there is one (np.maximum propagates it)
            total = np.maximum.reduceat(np.where(ok, v.astype(np.float64), -np.inf), self.heads)
        else:
            raise ValueError(func)
        return np.where(some, total, np.zeros(1, total.dtype)), some

    # ---- STRING_AGG
    def string_agg(self, values, separator: bytes):
        """``values``: ``bytes | None`` per input row.  ``(offsets int64[m + 1], data bytes, valid bool[m])``: the
        non-NULL members of a region in (start, row) order, joined by ``separator``; a region without one is NULL and
        holds no bytes; an empty string is a value and brings its separator."""
        vs = [values[i] for i in self.order.tolist()]
        ok = np.fromiter((v is not None for v in vs), bool, self.n)
        before = np.cumsum(ok) - ok                              # non-NULL members before a position ...
        lead = ok & (before == before[self.heads][self.region])  # ... none inside its region: it brings no separator
        lens = np.fromiter((0 if v is None else len(v) for v in vs), np.int64, self.n)
        size = np.where(ok, lens + np.where(lead, 0, len(separator)), 0)
        offsets = np.concatenate([[0], np.cumsum(np.add.reduceat(size, self.heads))]).astype(np.int64)
        data = b"".join(v if f else separator + v for v, k, f in zip(vs, ok.tolist(), lead.tolist()) if k)
        assert len(data) == offsets[-1]
        return offsets, data, np.add.reduceat(ok.astype(np.int64), self.heads) > 0

    def strings(self, values, separator: bytes):
        """``string_agg`` as a list of ``bytes | None`` per region."""
        off, data, ok = self.string_agg(values, separator)
        return [data[off[g]:off[g + 1]] if ok[g] else None for g in range(self.m)]
