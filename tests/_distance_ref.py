"""numpy restatement of DISTANCE and of the within-distance join, and the golden fixture's loader.

The value is the CASE of the reference (src/giql/expanders/_distance.py:67-117) on canonical 0-based half-open
coordinates, in int64::

    NULL                        when the chromosomes differ [stranded: or a strand is NULL / '.' / '?']
    0                           when a.start < b.end AND a.end > b.start
    +(b.start - a.end + 1)      when a.end <= b.start      (B downstream of A)
    +(a.start - b.end + 1)      otherwise                  (B upstream of A)

with the signs of the variant applied after the + 1: ``signed`` makes the upstream value negative, ``stranded``
negates whatever the value is when A's strand is '-' (so stranded + signed upstream on '-' is positive again).
The join is the value filtered, ``DISTANCE(a, b) <= N`` -- NOT the widened-overlap identity the kernels use, so the
two are independent statements of the same set.  numpy only."""

import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OFFSETS = {("0based", "half_open"): (0, 0), ("0based", "closed"): (0, 1),
           ("1based", "half_open"): (-1, -1), ("1based", "closed"): (-1, 0)}
VARIANTS = {"plain": (False, False), "signed": (False, True), "stranded": (True, False),
            "stranded_signed": (True, True)}
STRAND_CODE = {"+": 0, "-": 1, ".": 2, "?": 3, None: 4}     # execute._strand_codes


def golden():
    with open(os.path.join(HERE, "golden", "distance.json")) as f:
        return json.load(f)


def distance(ac, as_, ae, bc, bs, be, signed=False, stranded=False, strand_a=None, strand_b=None):
    """Elementwise DISTANCE of paired rows (canonical coordinates) -> ``(int64 values, bool valid)``."""
    ac, as_, ae, bc, bs, be = (np.asarray(x, np.int64) for x in (ac, as_, ae, bc, bs, be))
    valid = ac == bc
    minus = np.zeros(ac.shape, bool)
    if stranded:
        sa, sb = np.asarray(strand_a, np.int64), np.asarray(strand_b, np.int64)
        valid = valid & np.isin(sa, (0, 1)) & np.isin(sb, (0, 1))
        minus = sa == 1
    overlap = (as_ < be) & (ae > bs)
    down = ae <= bs
    d = np.where(overlap, 0, np.where(down, bs - ae + 1, as_ - be + 1))
    up = ~overlap & ~down
    if signed:
        d = np.where(up, -d, d)
    d = np.where(minus, -d, d)
    return np.where(valid, d, 0), valid


def sort_pairs(p):
    p = np.asarray(p, np.int64).reshape(-1, 2)
    return p[np.lexsort((p[:, 1], p[:, 0]))]


def window_pairs(ac, as_, ae, bc, bs, be, n):
    """Sorted ``[k, 2]`` (row_a, row_b) with equal chromosome and DISTANCE <= n; canonical coordinates."""
    ac, bc = np.asarray(ac, np.int64), np.asarray(bc, np.int64)
    if ac.size == 0 or bc.size == 0:
        return np.zeros((0, 2), np.int64)
    ia, ib = np.meshgrid(np.arange(ac.size), np.arange(bc.size), indexing="ij")
    ia, ib = ia.ravel(), ib.ravel()
    d, valid = distance(ac[ia], np.asarray(as_)[ia], np.asarray(ae)[ia], bc[ib], np.asarray(bs)[ib], np.asarray(be)[ib])
    keep = valid & (d <= n)
    return sort_pairs(np.stack([ia[keep], ib[keep]], 1))


def overlap_pairs(ac, as_, ae, bc, bs, be):
    ac, as_, ae, bc, bs, be = (np.asarray(x, np.int64) for x in (ac, as_, ae, bc, bs, be))
    m = (ac[:, None] == bc[None, :]) & (as_[:, None] < be[None, :]) & (ae[:, None] > bs[None, :])
    r, c = np.nonzero(m)
    return sort_pairs(np.stack([r, c], 1))


def case_arrays(case):
    """A random fixture case -> ``(side_a, side_b, n_chrom)``; a side = ``(codes, start, end, offsets, strand
    codes)`` with the coordinates in the table's declared encoding and one chromosome dictionary over both."""
    names = sorted({r[0] for r in case["a"]} | {r[0] for r in case["b"]})
    code = {n: i for i, n in enumerate(names)}

    def side(rows, enc):
        c = np.array([code[r[0]] for r in rows], np.int32)
        s = np.array([r[1] for r in rows], np.int32)
        e = np.array([r[2] for r in rows], np.int32)
        st = np.array([STRAND_CODE[r[3]] for r in rows], np.int32)
        return c, s, e, OFFSETS[tuple(enc)], st

    return side(case["a"], case["enc_a"]), side(case["b"], case["enc_b"]), len(names)


def canonical(side):
    c, s, e, (so, eo), _st = side
    return c, s.astype(np.int64) + so, e.astype(np.int64) + eo
