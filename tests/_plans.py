"""Compact plans without a GPU: the numpy expansion both plan test modules share, hand-built plans that aim at
each path of ``k_fill``, and a numpy mirror of ``k_partition`` / ``k_fill`` that says which path a plan takes.

A compact plan is four arrays: per query row ``q_rid[i]``, ``lo[i]``, ``cnt[i]`` and the other side's row ids
``s_rid`` in sorted order; pair ``k < cnt[i]`` of query row ``i`` is ``(q_rid[i], s_rid[lo[i] + k])``
(``include/giql_hip.h``, ``giql_hip_fill_from_plan_dev``).
"""

import numpy as np

# giql_amd/csrc/join_kernels.hip.h:1120-1124 (GIQL_FILL_NT, FILL_QCAP), giql_amd/csrc/giql_hip.hip:70-73
# (GIQL_FILL_ITEMS), join_kernels.hip.h:1187-1189 (a wave owns PER_WAVE consecutive outputs, 64 per window),
# giql_amd/csrc/scan.hip.h:11-13 (SCAN_TILE)
FILL_NT = 1024
FILL_ITEMS = 16
TILE = FILL_NT * FILL_ITEMS
FILL_QCAP = 4 * FILL_NT
WINDOW = 64
PER_WAVE = TILE // (FILL_NT // WINDOW)
SCAN_TILE = 4096

assert TILE == 16384 and FILL_QCAP == 4096 and PER_WAVE == 1024

PATHS = ("few", "mask", "slow", "search", "partial")


# ------------------------------------------------------------------ the reference
def expand_np(q_rid, lo, cnt, s_rid):
    """``(row_q, row_s)`` of a plan given as numpy arrays, in the kernel's order: pair k of row i at off[i] + k."""
    c = np.asarray(cnt).astype(np.int64)
    row_q = np.repeat(np.asarray(q_rid), c)
    start = np.repeat(np.asarray(lo).astype(np.int64), c)
    within = np.arange(int(c.sum())) - np.repeat(np.cumsum(c) - c, c)
    return row_q, np.asarray(s_rid)[start + within]


def _np_expand(q_rid, lo, cnt, s_rid, n_pairs):
    """numpy stand-in for giql_hip_fill_from_plan_dev (torch tensors in and out)."""
    import torch

    row_q, row_s = expand_np(q_rid.numpy(), lo.numpy(), cnt.numpy(), s_rid.numpy())
    assert row_q.shape[0] == n_pairs
    return torch.from_numpy(row_q.astype(np.int32)), torch.from_numpy(row_s.astype(np.int32))


def expand_loops(q_rid, lo, cnt, s_rid):
    """The same thing as the header words it: two plain loops."""
    row_q, row_s = [], []
    for i in range(len(q_rid)):
        for k in range(int(cnt[i])):
            row_q.append(int(q_rid[i]))
            row_s.append(int(s_rid[int(lo[i]) + k]))
    return row_q, row_s


def pair_words(row_q, row_s):
    """The pairs as sorted 64-bit words: the ids are opaque 32-bit words, negative ones included."""
    q = np.ascontiguousarray(row_q, np.int32).view(np.uint32).astype(np.uint64)
    s = np.ascontiguousarray(row_s, np.int32).view(np.uint32).astype(np.uint64)
    return np.sort((q << np.uint64(32)) | s)


# ------------------------------------------------------------------ which path of k_fill a plan takes
def classify(cnt):
    """What ``k_partition`` + ``k_fill`` do with these counts.  Returns a dict:

    ``total``, ``n_tiles``; ``tile_rows[t]`` = rows the tile spans (``part[t + 1] - part[t] + 1``, the kernel's
    ``nqt``); ``tile_path[t]`` in {"staged", "search"}; ``tile_partial[t]``; per 64-pair window of the staged tiles
    ``win_starts`` (rows that start in it, at most 64 candidates are looked at), ``win_dup`` (two of them share a
    start) and ``win_path`` in {"few", "mask", "slow"}; ``paths`` = the set of PATHS reached.
    """
    c = np.asarray(cnt).astype(np.int64)
    nq = c.shape[0]
    off = np.concatenate([[0], np.cumsum(c)])
    total = int(off[-1])
    nt = (total + TILE - 1) // TILE
    out = dict(total=total, n_tiles=nt, paths=set())
    if total == 0:
        out.update(tile_rows=np.zeros(0, np.int64), tile_path=[], tile_partial=np.zeros(0, bool),
                   win_starts=np.zeros(0, np.int64), win_dup=np.zeros(0, bool), win_path=[])
        return out
    # k_partition: part[t] = the last row whose offset is <= t * TILE; part[nt] = nq - 1 (join_kernels.hip.h:1141-1147)
    part = np.searchsorted(off, np.arange(nt + 1) * TILE, "right") - 1
    part[nt] = nq - 1
    part = np.minimum(part, nq - 1)
    rows = part[1:] - part[:-1] + 1
    staged = rows <= FILL_QCAP                               # k_fill: `fits` (first_delta stays far below 2^31 here)
    partial = (np.arange(nt) + 1) * TILE > total            # k_fill: tile_len < TILE
    # fill_wave: the candidates of a window are the rows after the row of the previous window's last output that
    # start before the window's end.  A wave's first window starts from the last row at or before its first output
    # (upper_bound at p_w0), so rows that start exactly there are not candidates.
    n_win = (total + WINDOW - 1) // WINDOW
    start = off[:nq]
    cand = np.nonzero((start % PER_WAVE != 0) & (start // WINDOW < n_win))[0]
    w = start[cand] // WINDOW
    rank = np.arange(cand.shape[0]) - np.searchsorted(w, w, "left")
    seen = rank < WINDOW                                     # 64 lanes look at 64 candidates
    starts = np.bincount(w[seen], minlength=n_win)
    same = np.zeros(cand.shape[0], bool)
    same[1:] = (start[cand][1:] == start[cand][:-1]) & (w[1:] == w[:-1])
    dup = np.bincount(w[seen & same], minlength=n_win) > 0
    win_tile = np.arange(n_win) * WINDOW // TILE
    path = np.where(starts <= 4, "few", np.where((starts < WINDOW) & ~dup, "mask", "slow"))
    path = np.where(staged[win_tile], path, "search")
    out.update(tile_rows=rows, tile_path=["staged" if s else "search" for s in staged], tile_partial=partial,
               win_starts=starts, win_dup=dup, win_path=path.tolist())
    out["paths"] = set(np.unique(path).tolist()) | ({"partial"} if partial.any() else set())
    return out


# ------------------------------------------------------------------ hand-built plans
N_S = 200_000


def build_plan(seed, cnt, n_s=N_S, lo=None, q_rid=None, q_add=7_000_000, s_add=1_000_000):
    """A plan around the counts ``cnt``: ``s_rid`` a random permutation of ``n_s`` ids plus an offset, ``q_rid``
    another one plus another offset, ``lo[i]`` uniform in ``[0, n_s - cnt[i]]`` unless given.  Every plan that
    leaves here keeps ``lo + cnt <= n_s``: the kernels do not check it."""
    r = np.random.default_rng(seed)
    cnt = np.asarray(cnt, np.int64)
    n_q = cnt.shape[0]
    assert n_q > 0 and int(cnt.min()) >= 0 and int(cnt.max()) <= n_s
    if lo is None:
        lo = r.integers(0, n_s - cnt + 1)
    lo = np.asarray(lo, np.int64)
    if q_rid is None:
        q_rid = r.permutation(n_q) + q_add
    s_rid = r.permutation(n_s) + s_add
    assert lo.shape == cnt.shape and int(lo.min()) >= 0 and bool(np.all(lo + cnt <= n_s))
    i32 = lambda x: np.ascontiguousarray(np.asarray(x, np.int64).astype(np.int32))
    return i32(q_rid), i32(lo), i32(cnt), i32(s_rid)


def _to_total(r, total, hi=9):
    """Counts uniform in 0..hi-1 whose sum is exactly ``total``."""
    c = r.integers(0, hi, 2 * total // (hi - 1) + 64)
    n = int(np.searchsorted(np.cumsum(c), total, "left")) + 1
    c = c[:n].copy()
    c[-1] -= int(c.sum()) - total
    assert int(c.sum()) == total and int(c.min()) >= 0
    return c


def plan_cases():
    """name -> (q_rid, lo, cnt, s_rid), int32 numpy arrays; EXPECT below names the path each case is built for."""
    r = np.random.default_rng(4242)
    cases = {}
    # 1. tiny: less than a handful of windows in all
    for n_q in (1, 2, 63, 64, 65):
        c = r.integers(0, 4, n_q)
        c[0] = max(int(c[0]), 1)
        cases[f"tiny_{n_q}"] = build_plan(10 + n_q, c)
    # 2. long rows: at most 4 rows start in a window
    cases["long_rows"] = build_plan(20, r.integers(16, 201, 12_000))
    # 3. medium rows: 5 to 16 starts per window, none shared
    cases["medium_rows"] = build_plan(30, r.integers(4, 13, 120_000))
    # 4. bursts: 71 consecutive starts cover a whole window, the tile stays far below FILL_QCAP rows
    cases["bursts"] = build_plan(40, np.tile(np.concatenate([np.ones(70, np.int64), [2000]]), 300))
    # 5. empty rows among full ones: shared starts inside windows
    c = r.integers(6, 41, 80_000)
    c[r.random(c.shape[0]) < 0.3] = 0
    cases["empty_among_full"] = build_plan(50, c)
    # 6. more rows in a tile than the LDS stage holds
    gap = np.zeros(FILL_QCAP + 400, np.int64)
    c = np.concatenate([np.zeros(5000, np.int64)] + [np.concatenate([[3000], gap]) for _ in range(40)]
                       + [np.zeros(5000 - gap.shape[0], np.int64)])
    cases["empty_runs"] = build_plan(60, c)
    cases["all_ones"] = build_plan(61, np.ones(3 * TILE + 17, np.int64))
    # 7. one giant row: tiles that lie wholly inside one row
    c = np.concatenate([r.integers(1, 9, 3000), [5 * TILE + 123], r.integers(1, 9, 3000)])
    cases["giant_row"] = build_plan(70, c)
    # 8. tile edges
    for name, total in (("total_tile", TILE), ("total_tile_minus_1", TILE - 1), ("total_tile_plus_1", TILE + 1),
                        ("total_two_tiles", 2 * TILE)):
        cases[name] = build_plan(80 + total % 7, _to_total(r, total))
    c = np.concatenate([_to_total(r, TILE), [0], r.integers(0, 9, 2000)])
    cases["row_ends_on_tile_then_empty"] = build_plan(85, c)
    # 9. plans another producer might send
    c = r.integers(0, 21, 30_000)
    n = c.shape[0]
    cases["same_lo"] = build_plan(90, c, lo=np.full(n, 1234))
    cases["descending_lo"] = build_plan(91, c, lo=np.sort(r.integers(0, N_S - 20, n))[::-1])
    cases["overlapping_ranges"] = build_plan(92, c, lo=r.integers(0, 50, n))
    cases["repeated_q_rid"] = build_plan(93, c, q_rid=r.integers(0, 100, n) + 5)
    cases["negative_ids"] = build_plan(94, c, q_add=-(1 << 31), s_add=-(N_S // 2))
    # 10. around the scan's tile
    for n_q in (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE + 1):
        cases[f"scan_{n_q}"] = build_plan(100 + n_q % 13, r.integers(0, 9, n_q))
    return cases


# the k_fill path every case is named for (checked on the CPU by test_compact_plan.py)
EXPECT = {
    "tiny_1": "partial", "tiny_2": "partial", "tiny_63": "partial", "tiny_64": "partial", "tiny_65": "partial",
    "long_rows": "few", "medium_rows": "mask", "bursts": "slow", "empty_among_full": "slow",
    "empty_runs": "search", "all_ones": "search", "giant_row": "few",
    "total_tile_minus_1": "partial", "total_tile_plus_1": "partial",
}
