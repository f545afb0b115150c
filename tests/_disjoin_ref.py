"""DISJOIN test helpers: the golden fixture and a brute-force restatement of the operator's semantics
(docs/dialect/set-operators.rst, DISJOIN; src/giql/expanders/disjoin.py:147-202)."""

import json
import os

import numpy as np

OFFSETS = {("0based", "half_open"): (0, 0), ("0based", "closed"): (0, 1),
           ("1based", "half_open"): (-1, -1), ("1based", "closed"): (-1, 0)}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "disjoin.json")


def golden_cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def brute_force(target, reference, encoding=("0based", "half_open")):
    """Sorted ``[target row, disjoin_start, disjoin_end]``.  ``target`` rows ``(chrom, start, end, ...)`` in
    ``encoding``; ``reference`` (None: self mode) canonical 0-based half-open."""
    so, eo = OFFSETS[tuple(encoding)]
    tgt = [(r[0], r[1] + so, r[2] + eo) for r in target]
    ref = tgt if reference is None else [(r[0], r[1], r[2]) for r in reference]
    out = []
    for i, (c, s, e) in enumerate(tgt):
        if s >= e:
            continue
        cuts = sorted({p for rc, rs, re_ in ref if rc == c for p in (rs, re_) if s < p < e})
        edges = [s] + cuts + [e]
        for x, y in zip(edges, edges[1:]):
            if reference is None or any(rc == c and rs <= x < re_ for rc, rs, re_ in ref):
                out.append([i, x - so, y - eo])
    return sorted(out)


def brute_force_arrays(t_chrom, t_start, t_end, r_chrom=None, r_start=None, r_end=None):
    """The same over canonical numpy columns, vectorised per chromosome (sort-based; for tables too large for
    the row-by-row form): sorted (parent, start, end) int64 array of shape [n, 3]."""
    self_mode = r_chrom is None
    if self_mode:
        r_chrom, r_start, r_end = t_chrom, t_start, t_end
    rows = []
    for c in np.unique(t_chrom):
        ti = np.nonzero(t_chrom == c)[0]
        rm = r_chrom == c
        rs, re_ = np.sort(r_start[rm]), np.sort(r_end[rm])
        bp = np.unique(np.concatenate([rs, re_]))
        depth = np.searchsorted(rs, bp, "right") - np.searchsorted(re_, bp, "right")   # rows with start <= bp < end
        s, e = t_start[ti], t_end[ti]
        lo, hi = np.searchsorted(bp, s, "right"), np.searchsorted(bp, e, "left")
        live = s < e
        n_cut = np.where(live, hi - lo, 0)
        # first piece
        first_end = np.where(n_cut > 0, bp[np.minimum(lo, max(len(bp) - 1, 0))] if len(bp) else e, e)
        first_cov = live if self_mode else live & (lo > 0) & (depth[np.maximum(lo - 1, 0)] > 0 if len(bp) else False)
        rows.append(np.stack([ti[first_cov], s[first_cov], first_end[first_cov]], 1))
        # pieces starting at a cut
        tot = int(n_cut.sum())
        if tot:
            owner = np.repeat(np.arange(len(ti)), n_cut)
            u = np.arange(tot) - np.repeat(np.cumsum(n_cut) - n_cut, n_cut) + lo[owner]
            nxt = np.where(u + 1 < hi[owner], bp[np.minimum(u + 1, len(bp) - 1)], e[owner])
            keep = np.ones(tot, bool) if self_mode else depth[u] > 0
            rows.append(np.stack([ti[owner][keep], bp[u][keep], nxt[keep]], 1))
    if not rows:
        return np.zeros((0, 3), np.int64)
    out = np.concatenate(rows).astype(np.int64)
    return out[np.lexsort((out[:, 2], out[:, 1], out[:, 0]))]
