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


# ---------------------------------------------------------------- constructed cases (tests/test_disjoin_paths.py)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "giql_amd", "csrc",
                      "disjoin_kernels.hip.h")
HALF_OPEN = ("0based", "half_open")


def fill_constants():
    """``DJ_FILL_TILE``, ``DJ_FILL_ITEMS`` and ``DJ_OFF_CAP`` as disjoin_kernels.hip.h defines them."""
    import re

    src = open(HEADER).read()

    def const(name):
        m = re.search(rf"constexpr\s+(?:int|u32)\s+{name}\s*=\s*([^;]+);", src)
        assert m, name
        return m.group(1).strip()

    nt, items = int(const("DJ_FILL_NT")), int(const("DJ_FILL_ITEMS"))
    assert const("DJ_FILL_TILE") == "DJ_FILL_NT * DJ_FILL_ITEMS"
    assert "make_int4(" in src and items == 4          # one 16-byte store holds DJ_FILL_ITEMS int32 slots
    return {"tile": nt * items, "items": items, "off_cap": int(const("DJ_OFF_CAP"))}


def fill_mirror(cnt, align=(0, 0, 0), consts=None):
    """What ``k_dj_fill`` does with the per-row piece counts ``cnt`` and outputs at the byte alignments ``align``
    (address mod 16 of parent / start / end), tile by tile, in plain numpy: the tile's slots ``[k0, k1)``, its first
    parent row ``r_lo`` and the ``nr`` rows up to its last parent, whether their offsets are staged in LDS
    (``nr <= DJ_OFF_CAP``), how many quads of ``DJ_FILL_ITEMS`` slots leave through the 16-byte store (``vec_quads``)
    and how many slot by slot (``scalar_quads``; ``partial``: the tile's last quad is cut by ``k1``), the slot of
    ``k0`` inside its parent row (``k0_in_row``: 0 when the parent's pieces start at the tile boundary) and the
    zero-piece rows among the tile's rows (``zero_rows``) and just past its last parent (``zero_after``)."""
    c = consts or fill_constants()
    tile, items, cap = c["tile"], c["items"], c["off_cap"]
    cnt = np.asarray(cnt, np.int64)
    n = len(cnt)
    off = np.concatenate([[0], np.cumsum(cnt)])[:n]      # exclusive offsets of the n rows
    total = int(cnt.sum())
    vec = all(a % 16 == 0 for a in align)
    tiles = []
    for k0 in range(0, total, tile):
        k1 = min(k0 + tile, total)
        r_lo = int(np.searchsorted(off, k0, "right")) - 1
        r_hi = int(np.searchsorted(off, k1 - 1, "right")) - 1
        quads = [(kt, min(kt + items, k1)) for kt in range(k0, k1, items)]
        n_vec = sum(1 for a, b in quads if vec and b - a == items)
        z_after = 0
        while r_hi + 1 + z_after < n and cnt[r_hi + 1 + z_after] == 0:
            z_after += 1
        tiles.append({"k0": k0, "k1": k1, "r_lo": r_lo, "nr": r_hi - r_lo + 1, "staged": r_hi - r_lo + 1 <= cap,
                      "vec_quads": n_vec, "scalar_quads": len(quads) - n_vec, "partial": (k1 - k0) % items != 0,
                      "k0_in_row": k0 - int(off[r_lo]), "zero_rows": int((cnt[r_lo:r_hi + 1] == 0).sum()),
                      "zero_after": z_after})
    return tiles


def tiles_of_row(cnt, row, consts=None):
    """The fill tiles that hold a piece of target row ``row``."""
    tile = (consts or fill_constants())["tile"]
    cnt = np.asarray(cnt, np.int64)
    a = int(cnt[:row].sum())
    return 0 if cnt[row] == 0 else (a + int(cnt[row]) - 1) // tile - a // tile + 1


class Case:
    """One DISJOIN call: raw int64 columns of each side in its declared encoding (``r`` None: self mode)."""

    def __init__(self, cid, t, r=None, n_chrom=1, t_enc=HALF_OPEN, r_enc=HALF_OPEN):
        self.id, self.n_chrom, self.t_enc, self.r_enc = cid, n_chrom, tuple(t_enc), tuple(r_enc)
        self.t = tuple(np.asarray(x, np.int64).reshape(-1) for x in t)
        self.r = None if r is None else tuple(np.asarray(x, np.int64).reshape(-1) for x in r)

    def __repr__(self):
        return self.id

    def canonical(self):
        so, eo = OFFSETS[self.t_enc]
        out = [self.t[0], self.t[1] + so, self.t[2] + eo]
        if self.r is not None:
            ro, re_ = OFFSETS[self.r_enc]
            out += [self.r[0], self.r[1] + ro, self.r[2] + re_]
        return out

    def expected(self):
        """``brute_force_arrays`` in the target's encoding: sorted (parent, start, end)."""
        so, eo = OFFSETS[self.t_enc]
        out = brute_force_arrays(*self.canonical())
        out[:, 1] -= so
        out[:, 2] -= eo
        return out

    def expected_row_by_row(self):
        """``brute_force`` (one target row at a time) on the same tables, the reference canonicalised for it."""
        t = list(zip(*(x.tolist() for x in self.t)))
        ref = None
        if self.r is not None:
            c = self.canonical()
            ref = list(zip(c[3].tolist(), c[4].tolist(), c[5].tolist()))
        return np.array(brute_force(t, ref, self.t_enc), np.int64).reshape(-1, 3)

    def counts(self):
        return np.bincount(self.expected()[:, 0], minlength=len(self.t[0])).astype(np.int64)


def case_from_counts(cid, cnt, seed=0, zero="mixed"):
    """Reference mode on one chromosome: target row i leaves exactly ``cnt[i]`` pieces.  The reference is a gap-free
    grid of max(cnt) book-ended cells of 3 to 6 bases from position 100 on; a row of c > 0 pieces starts and ends
    inside cells c - 1 apart (or on their edges), a row of no pieces is a zero-length row inside the grid, a live row
    below every breakpoint or a live row above every breakpoint (``zero``: "mixed" takes the three in turn)."""
    r = np.random.default_rng(seed)
    cnt = np.asarray(cnt, np.int64)
    g = max(int(cnt.max()), 1)
    edges = 100 + np.concatenate([[0], np.cumsum(r.integers(3, 7, g))])
    first = np.where(cnt > 0, r.integers(0, g - np.maximum(cnt, 1) + 1), 0)
    last = first + np.maximum(cnt, 1) - 1                                 # the row's last cell
    start = edges[first] + r.integers(0, 3, len(cnt))                    # on the cell's edge or up to 2 bases inside
    end = edges[last + 1] - r.integers(0, 2, len(cnt))                   # on the cell's end or 1 base before it
    kinds = {"mixed": np.arange(len(cnt)) % 3, "point": np.zeros(len(cnt), int), "below": np.ones(len(cnt), int),
             "above": np.full(len(cnt), 2)}[zero]
    top = int(edges[-1])
    for i in np.nonzero(cnt == 0)[0]:
        k = kinds[i]
        start[i], end[i] = ((edges[i % g], edges[i % g]), (10 + i % 40, 50 + i % 40), (top + 5 + i % 9, top + 30))[k]
    z = np.zeros(len(cnt), np.int64)
    return Case(cid, (z, start, end), (np.zeros(g, np.int64), edges[:-1], edges[1:]))


def path_cases(consts=None):
    """id -> (Case, the per-row counts it was built from): one case per path of ``k_dj_fill`` the issue names.
    ``test_disjoin.py`` shows on the CPU that each reaches its path (``fill_mirror``)."""
    c = consts or fill_constants()
    tile, cap = c["tile"], c["off_cap"]
    out = {}

    def add(cid, cnt, **kw):
        cnt = np.asarray(cnt, np.int64)
        out[cid] = (case_from_counts(cid, cnt, seed=len(out) + 1, **kw), cnt)

    gap = lambda n: [0] * n
    add("unstaged-5000", [1] + gap(5000) + [1])
    add("cap-exactly", [1] + gap(cap - 2) + [1])                 # cap rows in the tile: still staged
    add("cap-plus-one", [2] + gap(cap - 1) + [3])                # cap + 1 rows: searched in global memory
    add("unstaged-leading-trailing-zeros", gap(9) + [1] + gap(cap + 5) + [2] + gap(11))
    add("zero-rows-at-tile-edges", [tile - 5, 5] + gap(7) + [3, tile - 3] + gap(3) + [tile] + gap(2))
    add("unstaged-second-tile", [tile] + gap(3) + [1] + gap(cap + 9) + [5] + [7] * 150)
    for total in (1, 3, 4, 5, tile - 1, tile, tile + 1, 4 * tile - 1, 4 * tile + 1):
        rows, left = [], total
        k = 0
        while left:
            rows.append(min(left, 1 + (7 * k) % 61))
            left -= rows[-1]
            k += 1
        add(f"total-{total}", rows)
    add("parent-starts-at-tile-boundary", [tile // 2, tile // 2, 40, 3])
    add("parent-straddles-two-tiles", [tile - 10, 30, 6])
    add("parent-straddles-five-tiles", [5, 3 * tile + 2 + (tile - 6), 2, 1])   # slots 5 .. 4*tile+1: tiles 0-4
    for m in (1, 2, 3):
        add(f"total-mod-4-is-{m}", [tile, 16, 4 + m])
    return out


def _grid(n, step=10, at=0):
    s = at + np.arange(n, dtype=np.int64) * step
    return np.zeros(n, np.int64), s, s + step


def coverage_cases():
    """The coverage logic of ``k_dj_events`` .. ``k_dj_count``, one hand-built table pair per rule."""
    z = lambda n: np.zeros(n, np.int64)
    out = []
    t3 = (z(3), [0, 40, 100], [100, 60, 130])
    out.append(Case("zero-length-reference-rows-cut-never-cover", t3, (z(4), [10, 50, 50, 120], [10, 50, 50, 120])))
    out.append(Case("zero-length-beside-covering-rows", t3, (z(5), [5, 10, 50, 120, 90], [30, 10, 50, 120, 125])))
    out.append(Case("book-ended-reference-rows", (z(2), [0, 15], [45, 30]), (z(4), [0, 10, 20, 30], [10, 20, 30, 40])))
    r = np.random.default_rng(5)
    nest = np.arange(400, dtype=np.int64)
    ident_s, ident_e = np.full(600, 1000), np.full(600, 3000)
    ref = (z(1000), np.concatenate([ident_s, 1000 + nest]), np.concatenate([ident_e, 3000 - nest]))
    ts = r.integers(900, 3100, 60)
    out.append(Case("1000-identical-and-nested-reference-rows", (z(60), ts, ts + r.integers(0, 900, 60)), ref))
    bp = (z(3), [100, 200, 300], [200, 300, 400])
    out.append(Case("target-start-on-a-breakpoint", (z(3), [100, 200, 400], [150, 450, 460]), bp))
    out.append(Case("target-end-on-a-breakpoint", (z(3), [50, 150, 90], [100, 300, 400]), bp))
    out.append(Case("target-inside-one-reference-row", (z(2), [120, 201], [180, 299]), bp))
    out.append(Case("target-equal-to-a-reference-row", (z(3), [100, 200, 100], [200, 300, 400]), bp))
    out.append(Case("zero-length-targets", (z(5), [100, 150, 50, 400, 120], [100, 150, 50, 400, 180]), bp))
    out.append(Case("zero-length-targets-self", (z(5), [100, 150, 50, 400, 120], [100, 150, 50, 400, 180])))
    # chromosome 0's largest end (a target's) is one key below chromosome 1's smallest start (a reference row's)
    out.append(Case("largest-end-meets-next-chromosomes-smallest-start",
                    ([0, 0, 1, 1], [5, 60, 0, 3], [90, 90, 40, 9]), ([0, 1, 1, 0], [10, 0, 20, 70], [50, 30, 40, 80]), 2))
    out.append(Case("largest-end-meets-next-chromosomes-smallest-start-self",
                    ([0, 0, 1, 1, 2], [5, 60, 0, 0, 0], [90, 90, 40, 9, 7]), None, 3))
    out.append(Case("target-below-and-above-every-breakpoint", (z(4), [0, 500, 0, 50], [50, 600, 100, 500]), bp))
    for te, (tso, teo) in OFFSETS.items():
        for re_, (rso, reo) in OFFSETS.items():
            tc, ts_, tl = r.integers(0, 2, 40), r.integers(0, 300, 40), r.integers(0, 120, 40)
            rc, rs_, rl = r.integers(0, 2, 60), r.integers(0, 300, 60), r.integers(0, 30, 60)
            out.append(Case(f"encodings-{te[0]}-{te[1]}-x-{re_[0]}-{re_[1]}", (tc, ts_ - tso, ts_ + tl - teo),
                            (rc, rs_ - rso, rs_ + rl - reo), 2, te, re_))
    return out


def seeded_small_case(seed):
    """At most 300 rows a side: negative coordinates, zero-length rows on both sides, duplicate rows, book-ended
    rows, chromosomes on one side only; odd seeds in self mode.  Canonical columns (0-based half-open)."""
    r = np.random.default_rng(77_000 + seed)
    n_chrom = int(r.integers(1, 6))

    def side(n, only):
        c = r.integers(0, n_chrom, n)
        if n_chrom > 1:
            c[c == only] = (only + 1) % n_chrom                  # no row of this side on chromosome `only`
        s = r.integers(-120, 120, n)
        ln = r.integers(0, 60, n)
        ln[r.random(n) < 0.15] = 0                                # zero-length rows
        e = s + ln
        k = n // 4
        if k:
            src = r.integers(0, n, k)
            c[:k], s[:k], e[:k] = c[src], s[src], e[src]          # duplicate rows
            src = r.integers(0, n, k)
            c[k:2 * k], s[k:2 * k] = c[src], e[src]               # book-ended: starts where another row ends
            e[k:2 * k] = s[k:2 * k] + r.integers(0, 40, k)
        return c, s, e

    t = side(int(r.integers(1, 301)), int(r.integers(0, n_chrom)))
    ref = None if seed % 2 else side(int(r.integers(0, 301)), int(r.integers(0, n_chrom)))
    return Case(f"seeded-{seed}", t, ref, n_chrom)


# ---------------------------------------------------------------- the raw ABI (GPU tests): plan and fill as two calls
def plan_raw(eng, target, reference, n_chrom):
    """``giql_hip_disjoin_plan_dev`` on DeviceSides (or ready ``giql_side`` structs): (return code, n_out)."""
    import ctypes

    n = ctypes.c_int64(-1)
    ct = target.c_struct() if hasattr(target, "c_struct") else target
    cr = reference.c_struct() if hasattr(reference, "c_struct") else reference
    rc = eng._L.giql_hip_disjoin_plan_dev(eng._h, ctypes.byref(ct), ctypes.byref(cr) if cr is not None else None,
                                          int(n_chrom), ctypes.byref(n), eng._stream())
    eng._keepalive = (target, reference)
    return rc, int(n.value)


def fill_raw(eng, outs, capacity):
    """``giql_hip_disjoin_fill_dev`` into three int32 device tensors (None: a NULL pointer): the return code."""
    ptr = [None if o is None else o.data_ptr() for o in outs]
    return eng._L.giql_hip_disjoin_fill_dev(eng._h, ptr[0], ptr[1], ptr[2], int(capacity), eng._stream())
