"""Brute-force reference for column-to-column CONTAINS / WITHIN joins, and the golden fixture's loader.

The predicate is the reference's ``_column_join`` (src/giql/expanders/intersects.py:155-166) on canonical 0-based
half-open coordinates::

    X CONTAINS Y  <=>  X.chrom = Y.chrom AND X.start <= Y.start AND X.end >= Y.end
    X WITHIN Y    <=>  Y CONTAINS X

with no row shape excluded: zero-length and inverted rows follow the literal predicate.  numpy only; the oracle has
no containment."""

import functools
import json
import os
import re

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


# ------------------------------------------------------------------ a second, sort-based reference
def contain_pairs_sorted(oc, os_, oe, ic, is_, ie):
    """The same pairs as ``contain_pairs`` without the O(n*m) matrix, for tables it would take minutes on (anchored on
    it over seeded tables in tests/test_contain.py).  A regular inner row (start < end) inside an outer row starts in
    ``[outer.start, outer.end)``: one ``searchsorted`` range per outer row over the inner rows ordered by (chrom,
    start), expanded and filtered by the end.  The few inner rows with end <= start go through ``contain_pairs``."""
    oc, os_, oe = (np.asarray(x, np.int64) for x in (oc, os_, oe))
    ic, is_, ie = (np.asarray(x, np.int64) for x in (ic, is_, ie))
    if oc.size == 0 or ic.size == 0:
        return np.zeros((0, 2), np.int64)
    odd = np.nonzero(ie <= is_)[0]
    reg = np.nonzero(ie > is_)[0]
    out = []
    if odd.size:
        p = contain_pairs(oc, os_, oe, ic[odd], is_[odd], ie[odd])
        out.append(np.stack([p[:, 0], odd[p[:, 1]]], 1))
    if reg.size:
        comp = lambda c, x: c * (1 << 36) + (x + (1 << 34))
        order = reg[np.argsort(comp(ic[reg], is_[reg]), kind="stable")]
        keys = comp(ic[order], is_[order])
        lo = np.searchsorted(keys, comp(oc, os_), "left")
        cnt = np.maximum(np.searchsorted(keys, comp(oc, oe), "left") - lo, 0)
        total = int(cnt.sum())
        assert total < 1 << 27, "too many candidates for one expansion"
        rows = np.repeat(np.arange(oc.size), cnt)
        idx = order[np.repeat(lo, cnt) + np.arange(total) - np.repeat(np.cumsum(cnt) - cnt, cnt)]
        keep = ie[idx] <= oe[rows]
        out.append(np.stack([rows[keep], idx[keep]], 1))
    return sort_pairs(np.concatenate(out))


def truth(outer, inner, max_cells=10**9):
    """``contain_pairs``, one chromosome at a time (a pair shares its chromosome, so the matrices of two different
    ones hold nothing), wherever that brute force takes seconds; the sort-based reference past that."""
    oc, ic = np.asarray(outer[0], np.int64), np.asarray(inner[0], np.int64)
    shared = np.intersect1d(oc, ic)
    rows = [(np.nonzero(oc == c)[0], np.nonzero(ic == c)[0]) for c in shared]
    if sum(o.size * i.size for o, i in rows) > max_cells:
        return contain_pairs_sorted(*outer, *inner)
    out = [np.zeros((0, 2), np.int64)]
    for o, i in rows:
        p = contain_pairs(*(np.asarray(x)[o] for x in outer), *(np.asarray(x)[i] for x in inner))
        out.append(np.stack([o[p[:, 0]], i[p[:, 1]]], 1))
    return sort_pairs(np.concatenate(out))


# ------------------------------------------------------------------ the kernels' constants, read from the sources
def _source(name):
    with open(os.path.join(os.path.dirname(HERE), "giql_amd", "csrc", name)) as f:
        return f.read()


def _constant(text, pattern):
    return int(re.search(pattern, text).group(1))


@functools.lru_cache(maxsize=None)
def constants():
    ct, jk, host = _source("contain_kernels.hip.h"), _source("join_kernels.hip.h"), _source("giql_hip.hip")
    c = {n: _constant(ct, rf"constexpr int {n} = (\d+);") for n in ("CT_NT", "CT_ITEMS", "CT_QCAP")}
    c["WAVE"] = 64
    c["CT_TILE"] = c["CT_NT"] * c["CT_ITEMS"]
    c["RC_NT"] = _constant(jk, r"#define GIQL_RC_NT (\d+)")
    c["RC_LDS_CAP"] = _constant(jk, r"#define GIQL_RC_CAP (\d+)")
    c["RC_MARGIN"] = _constant(jk, r"constexpr int RC_MARGIN = (\d+);")
    c["RC_TQ"] = c["RC_NT"] * _constant(host, r"#define GIQL_RC_ITEMS (\d+)")
    return c


# ------------------------------------------------------------------ the general form's candidate tiles, in numpy
def _upper_bound(arr, lo, hi, x):
    """``upper_bound_u32(arr, lo, hi, x)`` of dev_common.hip.h for a vector of (lo, hi, x): the first index in
    [lo, hi) whose element is > x, ``hi`` when there is none."""
    lo, hi = np.array(lo, np.int64), np.array(hi, np.int64)
    while True:
        act = lo < hi
        if not act.any():
            return lo
        mid = (lo + hi) // 2
        right = act & (arr[np.minimum(mid, arr.size - 1)] <= x)
        lo = np.where(right, mid + 1, lo)
        hi = np.where(act & ~right, mid, hi)


def mirror_general_form(outer, inner, tile, qcap, n_waves=16, win=64):
    """The general form's index arithmetic restated in numpy (contain_kernels.hip.h, one chromosome: a key is a
    start).  ``outer`` / ``inner`` are (start, end) in input order; rows with end <= start carry the sentinel key: they
    sort last, own no candidates and are no candidates.  Candidate ranges of the sorted outer rows, u64 offsets,
    ``k_partition``, then per tile the staged row records -- relative start clamped to [0, tile_len], ``jbase = lo -
    (coff - tile base)`` modulo 2^32 -- and the per-wave walk: a wave owns ``tile / n_waves`` consecutive candidates
    and takes them ``win`` at a time; a lane finds the owner of its first candidate with ``upper_bound(rel, 1, nqt, p)
    - 1`` and steps forward for the next windows: ``if k + 1 < nqt and rel[k + 1] <= p: k = upper_bound(rel, k + 2,
    nqt, p) - 1``.  A tile of more than ``qcap`` rows searches the offsets themselves.  Then the test ``inner_end[j] <=
    outer_end[q]`` and a slot = tile offset + rank among the tile's passing candidates.

    Returns the regular pairs in slot order and one record per tile: ``nqt``, ``staged``, ``tile_len``, ``count``
    (passing candidates), ``owners`` (distinct owning rows of each ``win``-candidate window), ``on_row_start`` (windows
    that begin exactly on the first candidate of a row that starts inside the tile), and of row 0 ``row0_back`` (how
    many of its candidates lie before the tile) and ``row0_lo``."""
    (ok, oe_), (ik, ie_) = ((np.asarray(x, np.int64) for x in side) for side in (outer, inner))
    o_reg, i_reg = oe_ > ok, ie_ > ik
    oo = np.concatenate([np.nonzero(o_reg)[0][np.argsort(ok[o_reg], kind="stable")], np.nonzero(~o_reg)[0]])
    io = np.nonzero(i_reg)[0][np.argsort(ik[i_reg], kind="stable")]
    n_reg_o = int(o_reg.sum())
    qs, qe, ss, se = ok[oo], oe_[oo], ik[io], ie_[io]
    lo = np.searchsorted(ss, qs, "left")
    cand = np.searchsorted(ss, qe, "left") - lo
    lo[n_reg_o:], cand[n_reg_o:] = 0, 0
    assert (cand >= 0).all()
    coff = np.concatenate([[0], np.cumsum(cand)]).astype(np.int64)
    total = int(coff[-1])
    n_tiles = -(-total // tile)
    part = [int(np.searchsorted(coff, t * tile, "right")) - 1 for t in range(n_tiles)] + [len(qs) - 1]
    assert tile % (n_waves * win) == 0
    per_wave = tile // n_waves
    p_w0 = np.repeat(np.arange(n_waves) * per_wave, win)
    lane = np.tile(np.arange(win), n_waves)
    pairs, info = [], []
    for t in range(n_tiles):
        start = t * tile
        tile_len = min(tile, total - start)
        qf, ql = part[t], min(part[t + 1], len(qs) - 1)
        nqt = ql - qf + 1
        rows = np.arange(qf, ql + 1)
        off = coff[rows]
        p = np.arange(tile_len)
        if nqt <= qcap:
            rel = np.clip(off - start, 0, tile_len)
            jbase = (lo[rows] - (off - start)) % 2**32
            assert rel[0] == 0 and (rel[1:] >= 1).all()
            k = np.zeros(n_waves * win, np.int64)
            first = p_w0 < tile_len
            k[first] = _upper_bound(rel, np.ones(first.sum()), np.full(first.sum(), nqt), (p_w0 + lane)[first]) - 1
            owner = np.full(tile_len, -1, np.int64)
            for it in range(per_wave // win):
                p_rel = p_w0 + it * win + lane
                if it > 0:
                    step = (k + 1 < nqt) & (rel[np.minimum(k + 1, nqt - 1)] <= p_rel)
                    k[step] = _upper_bound(rel, k[step] + 2, np.full(step.sum(), nqt), p_rel[step]) - 1
                inside = p_rel < tile_len
                owner[p_rel[inside]] = k[inside]
            assert (owner >= 0).all()
            j = (jbase[owner] + p) % 2**32
            q = rows[owner]
            starts_here = np.isin(p[::win], rel[1:][cand[rows[1:]] > 0])
        else:
            q = np.searchsorted(coff[qf: ql + 1], start + p, "right") - 1 + qf
            j = lo[q] + (start + p - coff[q])
            starts_here = np.isin(start + p[::win], coff[qf + 1: ql + 1][cand[qf + 1: ql + 1] > 0])
        assert (j < len(ss)).all()
        passing = se[j] <= qe[q]
        pairs.append(np.stack([oo[q[passing]], io[j[passing]]], 1))
        change = np.concatenate([[0], (np.diff(q) != 0).astype(np.int64)])
        change[::win] = 0
        info.append({"nqt": nqt, "staged": nqt <= qcap, "tile_len": tile_len, "count": int(passing.sum()),
                     "owners": 1 + np.add.reduceat(change, np.arange(0, tile_len, win)),
                     "on_row_start": int(starts_here.sum()), "row0_back": int(start - coff[qf]), "row0_lo": int(lo[qf])})
    out = np.concatenate(pairs) if pairs else np.zeros((0, 2), np.int64)
    return out, info


# ------------------------------------------------------------------ the path cases of tests/test_contain_paths.py
class Case:
    """One chromosome-0 pair of tables in input (shuffled) order: ``outer`` / ``inner`` = (chrom, start, end)."""

    def __init__(self, cid, outer, inner, n_chrom=1, **notes):
        self.id, self.outer, self.inner, self.n_chrom, self.notes = cid, outer, inner, n_chrom, notes

    @functools.cached_property
    def want(self):
        return truth(self.outer, self.inner)

    @functools.cached_property
    def mirror(self):
        c = constants()
        return mirror_general_form(self.outer[1:], self.inner[1:], c["CT_TILE"], c["CT_QCAP"])

    def regular_pairs(self):
        """The wanted pairs between two regular rows: what the candidate tiles write (the first ``n_reg`` slots)."""
        w = self.want
        keep = (self.outer[2] > self.outer[1])[w[:, 0]] & (self.inner[2] > self.inner[1])[w[:, 1]]
        return w[keep]


def tables_from_counts(cid, counts, seed, orphans=None, covers=(), odd_outer=0, odd_inner=0, base=0):
    """Outer rows that tile the axis in the order given, row q owning exactly ``counts[q]`` candidates: inner rows with
    distinct starts ``outer.start + 2 i``.  ``orphans[q]`` inner rows lie in the gap before row q (inside no tiling
    row: they move ``lo`` without moving the candidate offsets).  About half of a row's candidates end inside it, a
    quarter of those exactly at its end; the others end 1 to 9 past it.  ``covers``: (first, last) pairs of tiling
    rows, each an extra outer row from the first one's start to the last one's end.  ``odd_outer`` rows with end <=
    start (half zero-length, half inverted), ``odd_inner`` zero-length inner rows (half of them equal to a zero-length
    outer row, the rest inside tiling rows).  Both tables are shuffled."""
    r = np.random.default_rng(seed)
    counts = np.asarray(counts, np.int64)
    n = counts.size
    orphans = np.zeros(n, np.int64) if orphans is None else np.asarray(orphans, np.int64)
    width = 2 * orphans + 2 * counts + 2
    os_ = base + np.cumsum(width) - width + 2 * orphans
    oe = os_ + 2 * counts + 1
    owner = np.repeat(np.arange(n), counts)
    nth = np.arange(owner.size) - np.repeat(np.cumsum(counts) - counts, counts)
    is_ = os_[owner] + 2 * nth
    u = r.random(owner.size)
    inside = np.minimum(is_ + 1 + r.integers(0, 40, owner.size), oe[owner])
    ie = np.where(u < 0.125, oe[owner], np.where(u < 0.5, inside, oe[owner] + 1 + r.integers(0, 9, owner.size)))
    orow = np.repeat(np.arange(n), orphans)
    onth = np.arange(orow.size) - np.repeat(np.cumsum(orphans) - orphans, orphans)
    orph_s = os_[orow] - 2 * orphans[orow] + 2 * onth
    orph_e = orph_s + 1 + r.integers(0, 30, orow.size)
    cs = np.array([os_[a] for a, _b in covers], np.int64)
    ce = np.array([oe[b] for _a, b in covers], np.int64)
    top = int(oe[-1]) + 50
    zs = top + 3 * np.arange(odd_outer)                       # past every inner start, apart from each other
    ze = np.where(np.arange(odd_outer) % 2 == 0, zs, zs - 1 - r.integers(0, 20, odd_outer))
    twins = zs[::2][: odd_inner // 2]                         # zero-length inner rows equal to zero-length outer rows
    held = os_[r.integers(0, n, odd_inner - twins.size)] if odd_inner else np.zeros(0, np.int64)
    o_s, o_e = np.concatenate([os_, cs, zs]), np.concatenate([oe, ce, ze])
    i_s, i_e = np.concatenate([is_, orph_s, twins, held]), np.concatenate([ie, orph_e, twins, held])
    po, pi = r.permutation(o_s.size), r.permutation(i_s.size)
    zeros = lambda k: np.zeros(k, np.int64)
    return Case(cid, (zeros(o_s.size), o_s[po], o_e[po]), (zeros(i_s.size), i_s[pi], i_e[pi]), 1,
                counts=counts, orphans=orphans)


DENSITIES = (0.25, 3, 64, 700, 5000)


def _density_case(mean):
    c = constants()
    r = np.random.default_rng(int(mean * 4) + 17)
    target = 3 * c["CT_TILE"] - 1111                           # about three tiles, the last one partial
    if mean < 100:
        counts = r.poisson(mean, int(target / mean) + 1)
    else:           # between half and one and a half times the mean, scaled to the target
        draws = r.integers(mean // 2, 3 * mean // 2, round(target / mean))
        counts = draws * target // int(draws.sum())
        counts[0] -= counts[0] % c["WAVE"]                     # row 1 begins exactly on a window
    counts[0] = max(counts[0], 1)
    return tables_from_counts(f"density-{mean}", counts, int(mean * 4) + 18)


def _qcap_case(extra, owning):
    """A first tile of exactly CT_QCAP + ``extra`` rows by the kernel's ``qf..ql`` rule, then a second, partial tile."""
    c = constants()
    tile, cap = c["CT_TILE"], c["CT_QCAP"]
    if owning:      # every row owns 4 candidates; row 0 owns 8 for the tile to end with row CT_QCAP - 1
        assert tile == 4 * cap
        counts = np.full(cap + 1500, 4)
        counts[0] = 8 if extra == 0 else 4
    else:           # two rows own 10,000 candidates each, the rows between them none (but for a few that own 1)
        counts = np.zeros(cap + 700, np.int64)
        counts[0] = counts[cap - 1 + extra] = 10_000
        counts[[5, 1000, cap - 2]] = 1
        counts[cap + extra:: 7] = 3
    return tables_from_counts(f"nqt-cap{'+1' if extra else ''}-{'all-own' if owning else 'most-own-none'}", counts,
                              40 + 2 * extra + owning)


def _trailing_case(odd):
    """About two and a half tiles of candidates, then CT_QCAP + 50 outer rows without candidates: regular rows past
    every inner start, or rows with end <= start, which sort last."""
    c = constants()
    n_trail = c["CT_QCAP"] + 50
    r = np.random.default_rng(60 + odd)
    counts = r.integers(0, 30, 2500)
    counts[::100] = 300
    if odd:
        return tables_from_counts("trailing-irregular", counts, 62, odd_outer=n_trail, odd_inner=40)
    return tables_from_counts("trailing-regular", np.concatenate([counts, np.zeros(n_trail, np.int64)]), 63)


def _straddle_case():
    """Seven rows of CT_TILE candidates each, 100 rows of 3 after every one of them and 9,000 candidates in front: each
    long row crosses a tile boundary and is row 0 of the tile it crosses into; 1,500 inner rows before the first
    outer row (and 7 before every long one) keep every ``lo`` well above its candidate offset."""
    c = constants()
    counts, orphans = [9000], [1500]
    for _ in range(7):
        counts += [3] * 100 + [c["CT_TILE"]]
        orphans += [0] * 100 + [7]
    counts += [3] * 120
    orphans += [0] * 120
    return tables_from_counts("straddle", counts, 70, orphans=orphans, covers=[(50, 260)])


def _uniform_case(L):
    """One chromosome, every inner row L long: 40,000 of them over [200, 24,000) (duplicated starts), 14,000 over
    [30,000, 3,000,000), six at the bottom.  Outer rows shorter than, equal to and longer than L everywhere; 1,500 over
    the dense part (a 512-row tile of theirs starts over more inner keys than the window stages), 2,000 over the
    sparse part with six rows 1,500,000 long among them (their ranges end past the staged window), and rows at the
    bottom of the axis whose end key is below L - 1."""
    r = np.random.default_rng(900 + L)
    i_s = np.concatenate([r.integers(200, 24_000, 40_000), r.integers(30_000, 3_000_000, 14_000), [0, 0, 1, 2, 3, 5]])

    def lengths(k):
        kind = r.integers(0, 3, k)
        return np.where(kind == 0, r.integers(1, max(L, 2), k), np.where(kind == 1, L, L + r.integers(1, 300, k)))

    d_s, s_s = r.integers(0, 24_000, 1500), r.integers(30_000, 3_000_000, 2000)
    d_e, s_e = d_s + lengths(1500), s_s + lengths(2000)
    s_e[:6] = s_s[:6] + 1_500_000
    b_s = np.array([0, 0, 1, 3, 0, 2])
    b_e = np.array([1, max(L - 2, 1), max(L - 3, 2), max(L - 2, 4), L, 2 + L])
    o_s, o_e = np.concatenate([b_s, d_s, s_s]), np.concatenate([b_e, d_e, s_e])
    po, pi = r.permutation(o_s.size), r.permutation(i_s.size)
    zeros = lambda k: np.zeros(k, np.int64)
    return Case(f"uniform-L{L}", (zeros(o_s.size), o_s[po], o_e[po]), (zeros(i_s.size), i_s[pi], i_s[pi] + L), 1, L=L)


def _sort_form_case(uniform):
    """About 20,000 rows a side on 3 chromosomes; the general set holds zero-length and inverted rows on both sides."""
    r = np.random.default_rng(1200 + uniform)
    n = 20_000
    oc, ic = r.integers(0, 3, n), r.integers(0, 3, n)
    o_s, i_s = r.integers(0, 2_000_000, n), r.integers(0, 2_000_000, n)
    o_e = o_s + r.integers(1, 30_000, n)
    i_e = i_s + (100 if uniform else r.integers(1, 20_000, n))
    if not uniform:
        for s, e, c in ((o_s, o_e, oc), (i_s, i_e, ic)):
            e[:50] = s[:50]
            e[50:100] = s[50:100] - 1 - r.integers(0, 30, 50)
        ic[:25], i_s[:25], i_e[:25] = oc[:25], o_s[:25], o_s[:25]       # [p, p) inside [p, p)
    return Case("sort-uniform" if uniform else "sort-general", (oc, o_s, o_e), (ic, i_s, i_e), 3)


PATH_CASES = {
    **{f"density-{m}": functools.partial(_density_case, m) for m in DENSITIES},
    "nqt-cap-all-own": functools.partial(_qcap_case, 0, True),
    "nqt-cap+1-all-own": functools.partial(_qcap_case, 1, True),
    "nqt-cap-most-own-none": functools.partial(_qcap_case, 0, False),
    "nqt-cap+1-most-own-none": functools.partial(_qcap_case, 1, False),
    "trailing-regular": functools.partial(_trailing_case, 0),
    "trailing-irregular": functools.partial(_trailing_case, 1),
    "straddle": _straddle_case,
    **{f"uniform-L{L}": functools.partial(_uniform_case, L) for L in (1, 2, 150)},
    "sort-general": functools.partial(_sort_form_case, 0),
    "sort-uniform": functools.partial(_sort_form_case, 1),
}
GENERAL_PATHS = [k for k in PATH_CASES if not k.startswith(("uniform", "sort"))]


@functools.lru_cache(maxsize=None)
def path_case(cid):
    case = PATH_CASES[cid]()
    assert case.id == cid
    return case


def sorted_uniform_ranges(case):
    """The uniform form's range count restated for a ``_uniform_case``: per 512-row outer tile the window start
    (``k_count_partition``), the staged length (``stage_window``) and per sorted outer row ``lo`` / ``hi`` with the
    shifted, clamped upper key."""
    c = constants()
    L = case.notes["L"]
    gmin = min(int(case.outer[1].min()), int(case.inner[1].min()))
    order = np.argsort(case.outer[1], kind="stable")
    qs, qe = case.outer[1][order] - gmin, case.outer[2][order] - gmin
    ss = np.sort(case.inner[1]) - gmin
    xe = np.maximum(qe + 1 - L, 0)
    lo = np.searchsorted(ss, qs, "left")
    hi = np.maximum(np.searchsorted(ss, xe, "left"), lo)
    nt = -(-qs.size // c["RC_TQ"])
    w_lo = np.concatenate([np.searchsorted(ss, qs[:: c["RC_TQ"]], "left"), [ss.size]])
    staged = np.minimum(np.minimum(ss.size - w_lo[:-1], np.diff(w_lo) + c["RC_MARGIN"]), c["RC_LDS_CAP"])
    tile_of = np.arange(qs.size) // c["RC_TQ"]
    return {"L": L, "qs": qs, "qe": qe, "lo": lo, "hi": hi, "w_lo": w_lo, "w_end": (w_lo[:-1] + staged)[tile_of],
            "owned": np.diff(w_lo), "tile_of": tile_of, "n_tiles": nt, "clamped": qe + 1 - L < 0}


def reach(cid):
    """What the case named ``cid`` is built to reach, asserted from the numpy restatements: the evidence the GPU tests
    of tests/test_contain_paths.py rest on (tests/test_contain.py runs it without a GPU)."""
    c = constants()
    case = path_case(cid)
    tile, cap = c["CT_TILE"], c["CT_QCAP"]
    if cid.startswith("uniform"):
        u = sorted_uniform_ranges(case)
        over = u["owned"] > c["RC_LDS_CAP"] + c["RC_MARGIN"]
        short = u["qe"] - u["qs"] < u["L"]
        ev = {"tiles_over_the_window": int(over.sum()),
              "rows_ending_past_a_whole_window": int(((u["hi"] > u["w_end"]) & ~over[u["tile_of"]]).sum()),
              "short_rows_past_the_window": int((short & (u["lo"] >= u["w_end"]) & (u["L"] > 1)).sum()),
              "clamped": int(u["clamped"].sum()),
              "duplicated_inner_starts": int(case.inner[1].size - np.unique(case.inner[1]).size)}
        lens = case.outer[2] - case.outer[1]
        assert case.inner[0].size >= 30_000 and ev["duplicated_inner_starts"] > 1000
        assert (lens == u["L"]).any() and (lens > u["L"]).any() and ((lens < u["L"]).any() or u["L"] == 1)
        assert ev["tiles_over_the_window"] >= 1 and 1 <= ev["rows_ending_past_a_whole_window"]
        if u["L"] > 1:
            assert ev["short_rows_past_the_window"] >= 1
        assert (ev["clamped"] >= 2) == (u["L"] == 150)         # an end key below L - 1 needs L >= 3
        return ev
    if cid.startswith("sort"):
        o, i = case.outer, case.inner
        ev = {"odd_outer": int((o[2] <= o[1]).sum()), "odd_inner": int((i[2] <= i[1]).sum())}
        assert o[0].size == i[0].size == 20_000 and set(o[0]) == set(i[0]) == {0, 1, 2}
        assert (len(set(i[2] - i[1])) == 1) == (cid == "sort-uniform")
        if cid == "sort-general":
            assert all(((s[2] == s[1]).sum() >= 50) and ((s[2] < s[1]).sum() >= 50) for s in (o, i))
        return ev
    pairs, info = case.mirror
    reg = case.regular_pairs()
    assert np.array_equal(sort_pairs(pairs), reg), cid
    total = sum(t["tile_len"] for t in info)
    ev = {"tiles": len(info), "T": total, "nqt": [t["nqt"] for t in info], "staged": [t["staged"] for t in info],
          "max_owners": max(int(t["owners"].max()) for t in info),
          "windows_on_a_row_start": sum(t["on_row_start"] for t in info), "pass_rate": reg.shape[0] / total}
    assert total % tile != 0 or cid == "nqt-cap-all-own"
    if cid.startswith("density"):
        mean = float(cid.split("-")[1])
        assert 2 < total / tile < 3 and abs(total / case.notes["counts"].size / mean - 1) < 0.1
        assert 0.2 < ev["pass_rate"] < 0.8 and all(0 < t["count"] < t["tile_len"] for t in info)
        assert ev["windows_on_a_row_start"] >= 1
        per_window = np.concatenate([t["owners"] for t in info])
        if mean <= 3:
            assert all(t["nqt"] > cap // 2 for t in info) and (mean > 1 or not any(ev["staged"]))
        if mean == 64:
            assert all(ev["staged"]) and (per_window[:-1] >= 2).mean() > 0.5
        if mean >= 700:       # a window holds one owner or two: the owner changes between windows
            assert all(ev["staged"]) and ev["max_owners"] <= 2 and (per_window == 1).mean() > 0.8
            assert len(np.unique(case.notes["counts"])) > 5 and ev["tiles"] * (tile // 64) > case.notes["counts"].size
    elif cid.startswith("nqt"):
        assert ev["nqt"][0] == cap + ("+1" in cid) and ev["staged"][0] == ("+1" not in cid) and ev["tiles"] >= 2
        owning = (case.notes["counts"][: cap] > 0).mean()
        assert owning == 1.0 if "all-own" in cid else owning < 0.01
    elif cid.startswith("trailing"):
        odd = cid == "trailing-irregular"
        o = case.outer
        n_odd = int((o[2] <= o[1]).sum())
        assert n_odd == (cap + 50 if odd else 0)
        if not odd:
            assert (case.notes["counts"][-(cap + 50):] == 0).all()
            assert np.sort(o[1])[-(cap + 50)] > case.inner[1].max()          # past every inner start
        assert not ev["staged"][-1] and ev["nqt"][-1] > cap + 50 and all(ev["staged"][:-1]) and ev["tiles"] >= 3
        ev["irregular_pairs"] = case.want.shape[0] - reg.shape[0]
        assert (ev["irregular_pairs"] > 0) == odd
    elif cid == "straddle":
        assert ev["tiles"] >= 7 and all(ev["staged"])
        crossed = [t for t in info[1:] if t["row0_back"] > 0 and t["row0_lo"] >= 1000 and t["nqt"] > 100]
        ev["tiles_entered_by_a_straddling_row"] = len(crossed)
        assert len(crossed) >= 6
        counts = case.notes["counts"]
        coff = np.concatenate([[0], np.cumsum(counts)])
        for b in range(1, 7):      # the tiling rows alone already cross every boundary (the cover row only adds)
            q = int(np.searchsorted(coff, b * tile, "right")) - 1
            assert counts[q] == tile and coff[q] < b * tile and (counts[q + 1: q + 101] == 3).all()
    return ev
