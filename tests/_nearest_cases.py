"""The tables of ``tests/test_nearest_paths.py`` and what the host can say about them without a GPU: the linear keys of both
layouts, the brackets ``k_nearest`` / ``k_nearest_k`` stage per block of A rows, the runs of equal keys the tie pass meets,
the oracle's brute force as truth (once per case and argument set).

Every case is seeded and small.  B holds no duplicate (chrom, start, end) row unless the case says so (``dups``): then a
row's neighbours are unique and the oracle's row ids are the only right answer.
"""
import functools
import os
import re

import numpy as np

from oracle import pyoracle as ora

HERE = os.path.dirname(os.path.abspath(__file__))

# the constants of giql_amd/csrc/aux_kernels.hip.h the cases are built around (test_cases_are_what_they_claim reads the
# header and fails when one of them moves: the case named there has to be rebuilt)
NR_TQ = 1024           # A rows per block (NR_NT * NR_ITEMS)
NR_CAP = 4096          # rows k_nearest stages
NRK_CAP = 2048         # rows k_nearest_k stages, per view
NR_BACK = 128          # rows staged below the bracket of the (start, end) view
NRK_EBACK = 192        # rows staged below the bracket of the (end, start) view
TIE_MAX = 32           # NEAREST_TIE_MAX: the longest run k_fix_start_ties orders in place
NR_CHROMS = 511        # chromosome tables in LDS up to this many chromosomes
MM_HIST_CHROMS = 32    # join_kernels.hip.h: the aligned layout (NEAREST's raw-column keys) up to this many chromosomes
CONSTANTS = {"NR_CAP": NR_CAP, "NRK_CAP": NRK_CAP, "NR_BACK": NR_BACK, "NRK_EBACK": NRK_EBACK, "NEAREST_TIE_MAX": TIE_MAX,
             "NR_CHROMS": NR_CHROMS, "NR_NT": 256, "MM_HIST_CHROMS": MM_HIST_CHROMS}


def header_constants():
    """name -> value as the kernels' headers define them."""
    out = {}
    for name in ("aux_kernels.hip.h", "join_kernels.hip.h"):
        with open(os.path.join(HERE, "..", "giql_amd", "csrc", name)) as f:
            text = f.read()
        for m in re.finditer(r"^constexpr (?:int|u32) (\w+) = (\d+)u?;", text, re.M):
            out[m.group(1)] = int(m.group(2))
        m = re.search(r"^#define GIQL_NR_ITEMS (\d+)", text, re.M)
        if m:
            out["GIQL_NR_ITEMS"] = int(m.group(1))
    return out


def side(c, s, e):
    return ora.Side(np.asarray(c, np.int32), np.asarray(s, np.int32), np.asarray(e, np.int32))


class Case:
    def __init__(self, cid, a, b, n_chrom, ks=(), dups=False, md=40, plan="one-sort", hand=None):
        self.id, self.a, self.b, self.n_chrom, self.dups, self._md, self.hand = cid, a, b, n_chrom, dups, md, hand
        self.ks = tuple(sorted({2, 16, *ks}))
        self.plan = plan                    # "one-sort" | "k-flags" (the (end, start) view's tie pass alone) | "all-flag"
        self.flags_1 = plan == "all-flag"   # nearest(), nearest32(), group_rows(): a run of equal starts above TIE_MAX
        self.flags_k = plan != "one-sort"   # nearest_k: that, or such a run of equal ends

    @property
    def md(self):
        """The case's small ``max_distance``; "median": the median of the oracle's unbounded distances."""
        if self._md == "median":
            idx, dist = self.nearest(False, None)
            self._md = int(np.median(np.abs(dist[idx >= 0])))
        return self._md

    # ------------------------------------------------------------ truth: the oracle's brute force, once
    @functools.lru_cache(maxsize=None)
    def nearest(self, signed, md):
        return ora.c_nearest_k1(self.a, self.b, signed=signed, max_distance=md, method="brute")

    @functools.lru_cache(maxsize=None)
    def nearest_k(self, k, signed=False, md=None):
        return ora.c_nearest_k(self.a, self.b, k, signed=signed, max_distance=md)

    @functools.lru_cache(maxsize=None)
    def groups(self):
        """(group of every B row, number of groups): ids ascending in (chrom, start, end) order."""
        trip = np.stack([self.b.chrom, self.b.start, self.b.end], 1).astype(np.int64)
        uniq, inv = np.unique(trip, axis=0, return_inverse=True)
        return inv.reshape(-1).astype(np.int64), len(uniq)

    # ------------------------------------------------------------ the linear axis
    @functools.lru_cache(maxsize=None)
    def aligned(self):
        """The layout with every chromosome base a multiple of 2^24 holds (``k_chrom_minmax``: ``aligned_ok``)."""
        if self.n_chrom > MM_HIST_CHROMS:
            return False
        buckets = 0
        for c in range(self.n_chrom):
            hi = [int(t.end[t.chrom == c].max()) for t in (self.a, self.b) if (t.chrom == c).any()]
            buckets += (max(hi) >> 24) + 1 if hi else 0
        return buckets <= 255

    @functools.lru_cache(maxsize=None)
    def keys(self, aligned):
        """(A start keys, A end keys, B start keys, B end keys) as int64 under the tight or the aligned layout."""
        base = np.zeros(self.n_chrom, np.int64)
        run = 0
        for c in range(self.n_chrom):
            both = [t for t in (self.a, self.b) if (t.chrom == c).any()]
            if not both:
                continue
            lo = min(int(t.start[t.chrom == c].min()) for t in both)
            hi = max(int(t.end[t.chrom == c].max()) for t in both)
            if aligned:
                base[c] = run << 24
                run += (hi >> 24) + 1
            else:
                base[c] = run - lo
                run += hi - lo + 1
        return tuple(base[t.chrom] + x.astype(np.int64) for t in (self.a, self.b) for x in (t.start, t.end))

    def layouts(self):
        return (False, True) if self.aligned() else (False,)

    def blocks(self, k=1):
        """Per block of NR_TQ A rows what the kernels compute from it, for A fully sorted and for A ordered by
        ``key >> 8`` / ``key >> 16`` with ties in input order (what ``row_skip`` may leave), under every layout the
        table can take: dicts of ``full`` (a block of NR_TQ rows), ``w_lo, w_hi`` (the bracket of lower_bound(B starts,
        a.end)), ``e_lo, e_hi`` (of upper_bound(B ends, a.start)), ``staged`` / ``staged_k`` / ``staged_e`` (the bracket
        is served from LDS in ``k_nearest``, in ``k_nearest_k`` with this ``k``, in its (end, start) view), ``e0``."""
        out = []
        for aligned in self.layouts():
            ak, ae, bk, be = self.keys(aligned)
            bs, bes = np.sort(bk), np.sort(be)
            nb = len(bs)
            for shift in (0, 8, 16):
                order = np.argsort(ak >> shift, kind="stable")
                for lo in range(0, len(order), NR_TQ):
                    rows = order[lo:lo + NR_TQ]
                    w_lo, w_hi = (int(np.searchsorted(bs, f(ae[rows]), "left")) for f in (np.min, np.max))
                    e_lo = int(np.searchsorted(bes, ak[rows].min(), "left"))
                    e_hi = int(np.searchsorted(bes, ak[rows].max(), "right"))
                    w0, e0 = max(w_lo - NR_BACK, 0), max(e_lo - NRK_EBACK, 0)
                    out.append(dict(full=len(rows) == NR_TQ, w_lo=w_lo, w_hi=w_hi, e_lo=e_lo, e_hi=e_hi, e0=e0, width=w_hi - w_lo,
                                    staged=min(w_hi + 1, nb) - w0 <= NR_CAP, staged_k=min(w_hi + k, nb) - w0 <= NRK_CAP,
                                    staged_e=e_hi - e0 <= NRK_CAP, shift=shift, aligned=aligned, first=lo == 0))
        return out

    def longest_runs(self):
        """(longest run of equal B start keys, of equal B end keys)."""
        return tuple(int(np.unique(np.stack([self.b.chrom, x], 1), axis=0, return_counts=True)[1].max())
                     for x in (self.b.start, self.b.end))

    def has_dups(self):
        return self.groups()[1] < self.b.n


# ---------------------------------------------------------------- builders
def _spread_duplicates(c, s, e, step):
    """Rows that repeat an earlier (chrom, start, end) get a longer end: the starts -- what the sort cases are about --
    and the number of rows stay."""
    e = e.copy()
    for _ in range(64):
        _u, first, inv, count = np.unique(np.stack([c, s, e], 1), axis=0, return_index=True, return_inverse=True, return_counts=True)
        inv = inv.reshape(-1)
        again = np.nonzero(first[inv] != np.arange(len(s)))[0]
        if len(again) == 0:
            return c, s, e
        e[again] += step * (1 + np.arange(len(again)) % 7)
    raise AssertionError("duplicates remain")


def _random_a(r, n, b, max_len=60):
    """n rows inside B's range, chromosome by chromosome (the span of the pair is B's)."""
    pick = r.integers(0, b.n, n)
    c = b.chrom[pick].astype(np.int64)
    lo = np.array([b.start[b.chrom == k].min() if (b.chrom == k).any() else 0 for k in range(int(b.chrom.max()) + 1)], np.int64)
    hi = np.array([b.end[b.chrom == k].max() if (b.chrom == k).any() else 1 for k in range(int(b.chrom.max()) + 1)], np.int64)
    s = lo[c] + (r.random(n) * (hi[c] - lo[c])).astype(np.int64)
    e = np.minimum(s + r.integers(0, max_len, n), hi[c])
    return side(c, s, e)


def _grouped_a(r, groups, max_len=30):
    """One chromosome.  ``groups``: (rows, lo, hi) -- that many rows with starts in [lo, hi), lo and hi - 1 among them.  Groups
    of NR_TQ rows in 2^16-key ranges of their own are the blocks of the kernels however the query side was sorted."""
    s = []
    for n, lo, hi in groups:
        g = r.integers(lo, hi, n)
        g[0], g[-1] = lo, hi - 1
        s.append(g)
    s = np.concatenate(s)[r.permutation(sum(g[0] for g in groups))]
    return side(np.zeros(len(s), np.int64), s, s + r.integers(0, max_len, len(s)))


def _ladder_b(r, n, step, max_len):
    """One chromosome, distinct starts 0, step, 2 * step, ... in random input order."""
    s = step * r.permutation(n).astype(np.int64)          # (one row in ten is long: the prefix maximum has plateaus)
    return side(np.zeros(n, np.int64), s, s + np.where(r.random(n) < 0.1, r.integers(1, max_len, n), r.integers(1, 8, n)))


def _runs_table(r, n, runs, by):
    """One chromosome of n rows whose ``by`` coordinates ("end" or "start") are 50 * i + 30, distinct, but for ``runs``:
    (p, L) gives rows p .. p + L - 1 the coordinate of row p and distinct other coordinates, in random input order."""
    x = 50 * np.arange(n, dtype=np.int64) + 30
    other = r.integers(1, 200, n)
    for p, L in runs:
        x[p:p + L] = x[p]
        other[p:p + L] = 1 + 3 * r.permutation(L)
    s, e = (np.maximum(x - other, 0), x) if by == "end" else (x, x + other)
    s[0] = 0
    order = r.permutation(n)
    return side(np.zeros(n, np.int64), s[order], e[order])


Q = 2721                       # the runs tables: rows by end before the second block of A (its smallest start: 50 * Q + 31)
S_BLOCK1 = 50 * Q + 31
SMALL_RUNS = [(p, 2 + p % 4) for p in range(100, Q - 300, 37)]


def _runs_a(r, right_of_b, probes=()):
    """1,024 rows over the first 2^16 keys, 48 rows in a block of their own from ``right_of_b`` on: twelve of them on it,
    ``probes`` (start, end) among them."""
    a = _grouped_a(r, [(NR_TQ, 0, 65_536), (48, right_of_b, right_of_b + 20_000)])
    late = np.nonzero(a.start >= right_of_b)[0]
    assert len(late) == 48 and len(probes) <= 30 and all(s >= right_of_b for s, _e in probes)
    a.end[late[:12]] += right_of_b - a.start[late[:12]]
    a.start[late[:12]] = right_of_b
    for i, (s, e) in zip(late[12:], probes):
        a.start[i], a.end[i] = s, e
    return a


RUN_START = 50 * (Q - 207) + 30        # the start-runs tables: the long run's start; probes inside its ends and up to it
START_PROBES = [(RUN_START + 3 * j + 2, RUN_START + 3 * j + 2 + j % 7) for j in range(0, 32, 2)] + \
               [(RUN_START - 10 - j, RUN_START - j) for j in range(4)]


HAND_A = [(0, 15, 25), (1, 100, 200), (2, 100, 100), (3, 10, 20)]
HAND_B = [(0, 0, 10), (0, 30, 40), (1, 50, 100), (1, 200, 300), (2, 100, 100), (3, 15, 30), (3, 20, 25), (3, 0, 4)]
# (k, signed, max_distance) -> per A row its (distance, start, end) rows, written by hand from the distance CASE: overlap 0;
# a.end <= b.start: b.start - a.end + 1 (downstream); else a.start - b.end + 1 (upstream, negative when signed); order
# ABS(distance), start, end -- so upstream comes first of two rows at one distance
HAND = {
    (1, False, None): [[(6, 0, 10)], [(1, 50, 100)], [(1, 100, 100)], [(0, 15, 30)]],
    (1, True, None): [[(-6, 0, 10)], [(-1, 50, 100)], [(1, 100, 100)], [(0, 15, 30)]],     # one point: downstream, +1
    (1, False, 6): [[(6, 0, 10)], [(1, 50, 100)], [(1, 100, 100)], [(0, 15, 30)]],
    (1, True, 5): [[], [(-1, 50, 100)], [(1, 100, 100)], [(0, 15, 30)]],
    (1, False, 0): [[], [], [], [(0, 15, 30)]],
    (2, False, None): [[(6, 0, 10), (6, 30, 40)], [(1, 50, 100), (1, 200, 300)], [(1, 100, 100)], [(0, 15, 30), (1, 20, 25)]],
    (2, True, None): [[(-6, 0, 10), (6, 30, 40)], [(-1, 50, 100), (1, 200, 300)], [(1, 100, 100)], [(0, 15, 30), (1, 20, 25)]],
    (2, False, 6): [[(6, 0, 10), (6, 30, 40)], [(1, 50, 100), (1, 200, 300)], [(1, 100, 100)], [(0, 15, 30), (1, 20, 25)]],
    (2, True, 5): [[], [(-1, 50, 100), (1, 200, 300)], [(1, 100, 100)], [(0, 15, 30), (1, 20, 25)]],
    (2, False, 0): [[], [], [], [(0, 15, 30)]],
    (3, True, None): [[(-6, 0, 10), (6, 30, 40)], [(-1, 50, 100), (1, 200, 300)], [(1, 100, 100)], [(0, 15, 30), (1, 20, 25), (-7, 0, 4)]],
}

SORT_SHAPES = ("rows-8191", "rows-8192", "rows-8193", "empty-and-one-row-buckets", "hot-bucket-above-bs-cap",
               "both-ends-of-the-axis", "20000-rows-sharing-200-starts")
PILE_UP = "sort/20000-rows-sharing-200-starts"
BLOCK_SIZES = (1, 1023, 1024, 1025, 2049)


@functools.lru_cache(maxsize=None)
def cases():
    """id -> Case, the ones that flag the two-sort plan last (a context keeps that plan)."""
    r = np.random.default_rng(2718)
    out = {}

    def add(cid, a, b, n_chrom, **kw):
        out[cid] = Case(cid, a, b, n_chrom, **kw)

    # 1 (and 4): blocks of 1, 1,023 ... 2,049 A rows over 3,000 B rows on three chromosomes; A keeps to a window of about
    # 1,600 B rows, so every bracket fits both stages -- until k = 2,100 carries the stage of k_nearest_k past its end
    c = np.repeat(np.arange(3), 1000)
    s = r.integers(0, 20_000_000, 3000)
    blocks_b = side(*_spread_duplicates(c, s, s + r.integers(1, 3000, 3000), 3001))
    ac = r.choice(3, 2049, p=[0.25, 0.625, 0.125])
    as_ = np.where(ac == 0, r.integers(12_000_000, 20_000_000, 2049), np.where(ac == 1, r.integers(0, 20_000_000, 2049),
                                                                               r.integers(0, 4_000_000, 2049)))
    ae = as_ + r.integers(0, 2000, 2049)
    for n in BLOCK_SIZES:
        add(f"blocks-{n}", side(ac[:n], as_[:n], ae[:n]), blocks_b, 3, ks=(15, 17, 2100) if n == 1025 else ())
    # 2: two full blocks whose brackets are about 2,850 rows: staged by k_nearest, read from global memory by k_nearest_k
    add("bracket-between-the-caps", _grouped_a(r, [(NR_TQ, 0, 57_000), (NR_TQ, 131_072, 131_072 + 57_000), (5, 262_144, 262_200)]),
        _ladder_b(r, 9_600, 20, 200), 1, md=0)
    # 3: one full block over 9,500 rows, five more rows in a block that stages
    add("bracket-wider-than-both", _grouped_a(r, [(NR_TQ, 0, 190_000), (5, 196_608, 230_000)]), _ladder_b(r, 12_000, 20, 200), 1, md=0)
    # 5: B's first row holds the largest end, 600 rows nested in it, every A row right of all of B
    s = np.sort(r.choice(np.arange(1, 50_000), 600, replace=False))
    gallop_b = side(np.zeros(601, np.int64), np.append(0, s), np.append(60_000, s + r.integers(1, 300, 600)))
    add("gallop-below-the-stage", _grouped_a(r, [(NR_TQ, 60_000, 65_536), (476, 65_536, 80_000)]), gallop_b, 1, ks=(300,), md=5000)
    # 6: runs of 2, 31 and exactly 32 equal ends (starts distinct) just below the second block's entry into the (end, start)
    # view -- the 32 across the lower edge e0 of its stage -- and short runs all over; k = 224 walks through all of them
    runs = SMALL_RUNS + [(Q - 207, 32), (Q - 40, 31), (Q - 3, 2)]
    add("end-runs-2-31-32", _runs_a(r, S_BLOCK1), _runs_table(r, Q + 1, runs, "end"), 1, ks=(224,), md=400)
    # 8: a run of 32 equal starts (ends distinct) does not flag; nor does one that holds two runs of equal rows
    runs = SMALL_RUNS + [(Q - 207, 32), (Q - 40, 31)]
    b = _runs_table(r, Q + 1, runs, "start")
    add("start-run-32", _runs_a(r, 50 * (Q - 215), START_PROBES), b, 1, md=400)
    e = b.end.copy()
    in_run = np.nonzero(b.start == 50 * (Q - 207) + 30)[0]
    e[in_run[3:8]], e[in_run[10:13]] = e[in_run[3]], e[in_run[10]]
    add("start-run-32-with-equal-rows", _runs_a(r, 50 * (Q - 215), START_PROBES), side(b.chrom, b.start, e), 1, dups=True, md=400)
    # 9: five chromosomes of 2^24 positions each (both layouts give the same keys), one block of A
    top = (1 << 24) - 1
    nine_b = [(0, 0, 7), (0, top - 5, top)] + [(0, top - 3000 + 9 * i, top - 2990 + 11 * i) for i in range(90)]                       # 0: B only, at its top
    nine_a = [(1, 0, 5)] + [(1, 20 * i + 3, 20 * i + 3 + i % 9) for i in range(200)]                                   # 1: A left of all of B
    nine_b += [(1, 9_000_000 + 700 * i, 9_000_000 + 700 * i + 300 + i) for i in range(149)] + [(1, top - 50, top)]
    nine_a += [(2, 0, 9), (2, top - 9, top)] + [(2, 70_000 * i + 11, 70_000 * i + 40) for i in range(1, 150)]          # 2: A only
    nine_b += [(3, 0, 4)] + [(3, 10_000 * i + 7, 10_000 * i + 7 + 900 + i) for i in range(1, 150)]                     # 3: A right of all of B
    nine_a += [(3, 11_000_000 + 30_000 * i, 11_000_000 + 30_000 * i + i % 13) for i in range(150)] + [(3, top - 4, top)]
    nine_b += [(4, 0, 10), (4, 500, 600)]                                                                          # 4: two B rows
    nine_a += [(4, 0, 0), (4, 3, 12), (4, 550, 700), (4, top - 1, top)] + [(4, 37 * i, 37 * i + i % 5) for i in range(300)]
    order = r.permutation(len(nine_a))
    nine_a = [nine_a[i] for i in order]
    order = r.permutation(len(nine_b))
    nine_b = [nine_b[i] for i in order]
    add("chromosome-clamps", side(*zip(*nine_a)), side(*zip(*nine_b)), 5, ks=(4,), md=3000)
    # 10: chromosome tables in LDS up to 511 chromosomes
    for n in (511, 512, 513):
        c = np.concatenate([np.arange(n), r.integers(0, n, n // 2)])
        s = r.integers(0, 100_000, len(c))
        b = side(*_spread_duplicates(c, s, s + r.integers(0, 500, len(c)), 501))
        c = np.concatenate([np.arange(n), r.integers(0, n, n // 2)])[r.permutation(n + n // 2)]
        s = r.integers(0, 100_000, len(c))
        add(f"chromosomes-{n}", side(c, s, s + r.integers(0, 500, len(c))), b, n, md=2000)
    # 11: the distance CASE's edges, expected rows by hand
    add("distance-edges", side(*zip(*HAND_A)), side(*zip(*HAND_B)), 4, hand=HAND, md=5)
    # 12: the tables of the CLUSTER / MERGE sort cases as B
    from test_one_table_paths import cases as sort_cases

    flagging = {}
    for name in SORT_SHAPES:
        t = sort_cases()[name]
        pile = name == "20000-rows-sharing-200-starts"
        table = (t.chrom, t.start, t.end) if pile or name == "both-ends-of-the-axis" else _spread_duplicates(t.chrom, t.start, t.end, 401)
        b = side(*table)
        (flagging if pile else out)["sort/" + name] = Case("sort/" + name, _random_a(r, 2000, b), b, t.n_chrom, dups=pile, md="median",
                                                           plan="all-flag" if pile else "one-sort")
    # 7: a run of 33 equal ends: NEAREST k > 1 alone leaves the one-sort plan
    runs = SMALL_RUNS + [(Q - 207, 33), (Q - 40, 31), (Q - 3, 2)]
    add("end-run-33", _runs_a(r, S_BLOCK1), _runs_table(r, Q + 1, runs, "end"), 1, md=400, plan="k-flags")
    # 8: a run of 33 equal starts: every operator of the family leaves it
    runs = SMALL_RUNS + [(Q - 207, 33), (Q - 40, 31)]
    add("start-run-33", _runs_a(r, 50 * (Q - 215), START_PROBES), _runs_table(r, Q + 1, runs, "start"), 1, md=400, plan="all-flag")
    out.update(flagging)
    return out


def same_rows(b, got_idx, got_dist, want_idx, want_dist, exact, what):
    """NEAREST rows as (distance, start, end) per A row and slot, in order; which slots are -1; with ``exact`` the row
    ids themselves (a B without duplicates leaves no tie)."""
    assert got_idx.shape == want_idx.shape and got_dist.shape == want_dist.shape, (what, got_idx.shape, want_idx.shape)
    ok = want_idx >= 0
    assert np.array_equal(got_idx >= 0, ok), (what, "which slots are -1", int(np.sum((got_idx >= 0) != ok)))
    bad = np.nonzero(got_dist != want_dist)
    assert len(bad[0]) == 0, (what, "distance", [x[:3].tolist() for x in bad], got_dist[bad][:3], want_dist[bad][:3])
    for name, col in (("start", b.start), ("end", b.end)):
        bad = np.nonzero(col[got_idx[ok]] != col[want_idx[ok]])[0]
        assert len(bad) == 0, (what, name, len(bad), col[got_idx[ok]][bad][:3], col[want_idx[ok]][bad][:3])
    if exact:
        assert np.array_equal(got_idx, want_idx), (what, "row ids")


def triples(idx, dist, b):
    return [[(int(dist[i, t]), int(b.start[idx[i, t]]), int(b.end[idx[i, t]])) for t in range(idx.shape[1]) if idx[i, t] >= 0]
            for i in range(idx.shape[0])]


def assert_groups(chrom, start, end, gid, rep, what=""):
    """``HipEngine.group_rows`` in full: ``gid`` is the inverse of ``np.unique`` over the (chrom, start, end) rows exactly --
    ids ascending in that order -- and ``rep[g]`` is a row of group g."""
    gid, rep = np.asarray(gid), np.asarray(rep)
    trip = np.stack([chrom, start, end], 1).astype(np.int64)
    if len(trip) == 0:
        assert gid.shape == (0,) and rep.shape == (0,), what
        return
    uniq, inv = np.unique(trip, axis=0, return_inverse=True)
    assert rep.shape == (len(uniq),), (what, "groups", rep.shape, len(uniq))
    assert gid.shape == (len(trip),) and np.array_equal(gid, inv.reshape(-1)), (what, "group_of_row")
    assert rep.min() >= 0 and rep.max() < len(trip) and np.array_equal(gid[rep], np.arange(len(uniq))), (what, "rep_row")
