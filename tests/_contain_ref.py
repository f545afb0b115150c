"""Brute-force reference for column-to-column CONTAINS / WITHIN joins, and the golden fixture's loader.

The predicate is the reference's ``_column_join`` (src/giql/expanders/intersects.py:155-166) on canonical 0-based
half-open coordinates::

    X CONTAINS Y  <=>  X.chrom = Y.chrom AND X.start <= Y.start AND X.end >= Y.end
    X WITHIN Y    <=>  Y CONTAINS X

with no row shape excluded: zero-length and inverted rows follow the literal predicate.  numpy only; the oracle has
no containment."""

import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OFFSETS = {("0based", "half_open"): (0, 0), ("0based", "closed"): (0, 1),
           ("1based", "half_open"): (-1, -1), ("1based", "closed"): (-1, 0)}


def golden_cases():
    with open(os.path.join(HERE, "golden", "contains_within.json")) as f:
        return json.load(f)["cases"]


def contain_pairs(oc, os_, oe, ic, is_, ie, chunk: int = 1 << 22):
    """Sorted ``[n, 2]`` int64 array of (outer row, inner row) with the inner row inside the outer one; canonical
    coordinates.  Outer rows are taken a block at a time so the boolean matrix stays at ``chunk`` cells."""
    oc, os_, oe = (np.asarray(x, np.int64) for x in (oc, os_, oe))
    ic, is_, ie = (np.asarray(x, np.int64) for x in (ic, is_, ie))
    if oc.size == 0 or ic.size == 0:
        return np.zeros((0, 2), np.int64)
    step = max(1, chunk // ic.size)
    out = []
    for lo in range(0, oc.size, step):
        hi = min(oc.size, lo + step)
        m = ((oc[lo:hi, None] == ic[None, :]) & (os_[lo:hi, None] <= is_[None, :]) & (oe[lo:hi, None] >= ie[None, :]))
        r, c = np.nonzero(m)
        out.append(np.stack([r + lo, c], axis=1))
    return sort_pairs(np.concatenate(out))


def sort_pairs(p):
    p = np.asarray(p, np.int64).reshape(-1, 2)
    return p[np.lexsort((p[:, 1], p[:, 0]))]


def overlap_pairs(ac, as_, ae, bc, bs, be):
    """The INTERSECTS pairs of the same tables (canonical): what a test compares a containment result with."""
    ac, as_, ae, bc, bs, be = (np.asarray(x, np.int64) for x in (ac, as_, ae, bc, bs, be))
    m = (ac[:, None] == bc[None, :]) & (as_[:, None] < be[None, :]) & (ae[:, None] > bs[None, :])
    r, c = np.nonzero(m)
    return sort_pairs(np.stack([r, c], axis=1))


def case_arrays(case):
    """A fixture case as ``(codes_a, start_a, end_a, offsets_a, codes_b, start_b, end_b, offsets_b, n_chrom)`` with the
    coordinates in each table's declared encoding and one chromosome dictionary over both."""
    names = sorted({r[0] for r in case["a"]} | {r[0] for r in case["b"]})
    code = {n: i for i, n in enumerate(names)}

    def side(rows):
        t = np.array([[code[r[0]], r[1], r[2]] for r in rows], np.int64).reshape(-1, 3)
        return t[:, 0].astype(np.int32), t[:, 1].astype(np.int32), t[:, 2].astype(np.int32)

    return (*side(case["a"]), OFFSETS[tuple(case["enc_a"])], *side(case["b"]), OFFSETS[tuple(case["enc_b"])], len(names))


def case_brute_force(case, predicate: str):
    """``a <predicate> b`` over a fixture case as sorted ``[[row_a, row_b], ...]``."""
    ac, as_, ae, (aso, aeo), bc, bs, be, (bso, beo), _ = case_arrays(case)
    a = (ac, as_.astype(np.int64) + aso, ae.astype(np.int64) + aeo)
    b = (bc, bs.astype(np.int64) + bso, be.astype(np.int64) + beo)
    if predicate == "contains":
        return contain_pairs(*a, *b).tolist()
    inner_outer = contain_pairs(*b, *a)          # (row_b, row_a) with a inside b
    return sort_pairs(inner_outer[:, ::-1]).tolist()
