"""Coverage-segment test helpers: two restatements of ``SELECT disjoin_chrom, disjoin_start, disjoin_end, COUNT(*)
FROM DISJOIN(t) GROUP BY`` the three, and of the run form ``MERGE(interval, predicate := depth = PREV(depth))`` over
those segments (docs/recipes/clustering.rst, "Reconstruct disjoin() Coverage Segments").

Definition, on canonical (0-based half-open) coordinates: per chromosome, ``bp`` = the distinct starts and ends; for
consecutive breakpoints x < y, ``depth(x)`` = the rows with start <= x < end; the segment [x, y) exists when
depth(x) > 0.  Runs: maximal runs of abutting segments of equal depth.  Both functions take and return rows in the
table's declared encoding and order the result by (chrom, start)."""

import json
import os

import numpy as np

from _disjoin_ref import OFFSETS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coverage.json")


def golden_cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def _runs_of(segments):
    """Abutting (canonical end == next canonical start, same chromosome) segments of equal depth, merged.  Rows
    ``[chrom, start, end, depth]`` canonical, ordered."""
    out = []
    for c, s, e, d in segments:
        if out and out[-1][0] == c and out[-1][2] == s and out[-1][3] == d:
            out[-1][2] = e
        else:
            out.append([c, s, e, d])
    return out


def sweep(rows, encoding=("0based", "half_open"), runs=False):
    """Row by row: ``rows`` = ``(chrom, start, end)`` in ``encoding``; returns ``[[chrom, start, end, depth], ...]``
    in ``encoding``.  One chromosome at a time, one breakpoint at a time, counting the covering rows."""
    so, eo = OFFSETS[tuple(encoding)]
    canon = [(r[0], r[1] + so, r[2] + eo) for r in rows]
    out = []
    for c in sorted({r[0] for r in canon}):
        mine = [(s, e) for rc, s, e in canon if rc == c]
        bp = sorted({p for s, e in mine for p in (s, e)})
        for x, y in zip(bp, bp[1:]):
            depth = sum(1 for s, e in mine if s <= x < e)
            if depth > 0:
                out.append([c, x, y, depth])
    if runs:
        out = _runs_of(out)
    return [[c, s - so, e - eo, d] for c, s, e, d in out]


def sweep_arrays(chrom, start, end, encoding=("0based", "half_open"), runs=False):
    """The same, vectorised per chromosome with ``searchsorted`` (as ``_disjoin_ref.brute_force_arrays`` derives the
    depth): int64 array of shape [m, 4]."""
    so, eo = OFFSETS[tuple(encoding)]
    chrom = np.asarray(chrom, np.int64)
    cs, ce = np.asarray(start, np.int64) + so, np.asarray(end, np.int64) + eo
    parts = []
    for c in np.unique(chrom):
        s, e = np.sort(cs[chrom == c]), np.sort(ce[chrom == c])
        bp = np.unique(np.concatenate([s, e]))
        depth = np.searchsorted(s, bp[:-1], "right") - np.searchsorted(e, bp[:-1], "right")
        seg = np.stack([np.full(depth.size, c, np.int64), bp[:-1], bp[1:], depth], 1)[depth > 0]
        if runs and len(seg):
            cont = (seg[1:, 1] == seg[:-1, 2]) & (seg[1:, 3] == seg[:-1, 3])
            head = np.concatenate([[True], ~cont])
            tail = np.concatenate([~cont, [True]])
            seg = np.stack([seg[head, 0], seg[head, 1], seg[tail, 2], seg[head, 3]], 1)
        parts.append(seg)
    out = np.concatenate(parts) if parts else np.zeros((0, 4), np.int64)
    out = out.astype(np.int64).reshape(-1, 4)
    out[:, 1] -= so
    out[:, 2] -= eo
    return out


def group_pieces(chroms, pieces):
    """DISJOIN's pieces ``[parent, start, end]`` grouped by (chromosome of the parent, start, end): sorted
    ``[chrom, start, end, count]`` -- the recipe's GROUP BY, restated."""
    counts = {}
    for parent, s, e in pieces:
        key = (chroms[parent], s, e)
        counts[key] = counts.get(key, 0) + 1
    return [[c, s, e, n] for (c, s, e), n in sorted(counts.items())]


def seeded_table(seed):
    """A small table that piles up: a coarse grid (many shared breakpoints), duplicates, nested rows, zero-length
    rows, 1 to 4 chromosomes, negative coordinates.  Canonical columns."""
    r = np.random.default_rng(91_000 + seed)
    n = int(r.integers(1, 120))
    n_chrom = int(r.integers(1, 5))
    step = int(r.choice([1, 5, 10]))
    c = r.integers(0, n_chrom, n)
    s = r.integers(-12, 30, n) * step
    ln = r.integers(0, 12, n) * step
    ln[r.random(n) < 0.15] = 0
    e = s + ln
    k = n // 4
    if k:
        src = r.integers(0, n, k)
        c[:k], s[:k], e[:k] = c[src], s[src], e[src]                      # duplicates
        src = r.integers(0, n, k)
        c[k:2 * k], s[k:2 * k], e[k:2 * k] = c[src], s[src] + step, np.maximum(e[src] - step, s[src] + step)  # nested
    return c.astype(np.int64), s.astype(np.int64), e.astype(np.int64), n_chrom


# ---------------------------------------------------------------- constructed tables (tests/test_coverage_gpu.py)
def shaped_table(kind, n):
    """One chromosome, ``n`` rows, canonical int64 columns ``(chrom, start, end)`` of the named shape."""
    i = np.arange(n, dtype=np.int64)
    z = np.zeros(n, np.int64)
    if n == 0 and kind in SHAPES:
        return z, z.copy(), z.copy()
    if kind == "distinct":           # 2n breakpoints
        return z, 3 * i, 3 * i + 3 * n + 1 + (i % 2)
    if kind == "identical":           # one segment of depth n
        return z, z + 7, z + 19
    if kind == "chain":               # n segments of depth 1, ONE run
        return z, 10 * i, 10 * i + 10
    if kind == "alternating":         # chain with every odd cell doubled: depth 1, 2, 1, 2, no two segments merge
        return _alternating(n)
    if kind == "nested":              # a staircase up to n and down
        return z, i, 2 * n - i
    if kind == "points":              # zero-length rows only
        return z, 5 * i, 5 * i
    if kind == "points-inside":       # long rows with zero-length rows strictly inside: cuts, depth unchanged
        k = max(n // 3, 1)
        long_s = 100 * np.arange(k, dtype=np.int64)
        pts = 100 * (np.arange(n - k, dtype=np.int64) % k) + 10 + 7 * (np.arange(n - k, dtype=np.int64) // k % 11)
        return z, np.concatenate([long_s, pts]), np.concatenate([long_s + 90, pts])
    raise KeyError(kind)


def _alternating(n):
    """Cells [10j, 10j + 10); every odd cell is covered twice: rows take the cells 0, 1, 1, 2, 3, 3, 4, ...  A last
    odd cell that would be left with one row gives that row to the odd cell before it (depth 3) instead."""
    j = np.arange(n, dtype=np.int64)
    cell = 2 * (j // 3) + (j % 3 + 1) // 2
    if n % 3 == 2:
        cell[-1] = cell[-3] if n >= 3 else 0
    return np.zeros(n, np.int64), 10 * cell, 10 * cell + 10


SHAPES = ("distinct", "identical", "chain", "alternating", "nested", "points", "points-inside")


# ---------------------------------------------------------------- the raw ABI (GPU tests)
def coverage_raw(eng, side, n_chrom, flags, outs, capacity):
    """``giql_hip_coverage_dev`` on a DeviceSide into four device tensors (None: a NULL pointer): (return code,
    n_out)."""
    import ctypes

    n = ctypes.c_int64(-1)
    ptr = [None if o is None else o.data_ptr() for o in outs]
    rc = eng._L.giql_hip_coverage_dev(eng._h, side.c_struct(), int(n_chrom), int(flags), ptr[0], ptr[1], ptr[2], ptr[3],
                                      int(capacity), ctypes.byref(n), eng._stream())
    eng._keepalive = (side,)
    return rc, int(n.value)
