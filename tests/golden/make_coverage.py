#!/usr/bin/env python3
"""Mint tests/golden/coverage.json: coverage-profile cases with their expected rows.  Standard library only.

``segments``: sqlite3 (>= 3.25) executes the CTE pipeline the reference emits for self-mode DISJOIN, as
make_disjoin.py restates it (src/giql/expanders/disjoin.py:147-202), wrapped in the recipe's GROUP BY
(docs/recipes/clustering.rst, "Reconstruct disjoin() Coverage Segments"):

    SELECT disjoin_chrom AS chrom, disjoin_start AS start, disjoin_end AS end, COUNT(*) AS depth
    FROM DISJOIN(features) GROUP BY disjoin_chrom, disjoin_start, disjoin_end

``runs`` (half-open targets only; ``null`` otherwise): the recipe's outer ``MERGE(interval, predicate := depth =
PREV(depth))`` over those rows -- sqlite3 executes the window SQL the reference emits for it, the adjacency CASE with
the predicate ANDed in and a GROUP BY over the cluster ids, as make_cluster_predicate.py restates it
(src/giql/expanders/cluster.py:210-300, merge.py:201-330).  Each run carries the depth its segments share.

A case: ``encoding``, ``rows`` as ``[chrom, start, end]`` in that encoding, ``segments`` and ``runs`` as
``[chrom, start, end, depth]`` ordered by (chrom, start).  No row has start > end.

    python tests/golden/make_coverage.py
"""

import json
import os
import random
import sqlite3

from make_disjoin import OFFSETS, PIPELINE

HERE = os.path.dirname(os.path.abspath(__file__))

PIECES = PIPELINE.format(ref="tgt", coverage="").replace("SELECT t.rid, s.seg_start, s.seg_end",
                                                          "SELECT t.chrom AS chrom, s.seg_start AS ps, s.seg_end AS pe")
SEGMENTS = ('SELECT chrom, ps - {so} AS "start", pe - {eo} AS "end", COUNT(*) AS depth FROM (' + PIECES +
            ") GROUP BY chrom, ps, pe ORDER BY chrom, ps")

_PART = 'PARTITION BY "chrom"'
_EDGE = f'MAX("end") OVER ({_PART} ORDER BY "start" NULLS LAST ROWS BETWEEN UNBOUNDED PRECEDING AND 1 PRECEDING)'
_LAG = f'LAG("depth") OVER ({_PART} ORDER BY "start" NULLS LAST)'
CLUSTERED = (f'SELECT *, SUM(__giql_is_new_cluster) OVER ({_PART} ORDER BY "start" NULLS LAST) AS __giql_cluster_id FROM ('
             f'SELECT *, CASE WHEN {_EDGE} >= "start" AND ("depth" = {_LAG}) THEN 0 ELSE 1 END AS __giql_is_new_cluster '
             "FROM segments) AS __giql_lag_calc")
RUNS = (f'SELECT "chrom", MIN("start"), MAX("end"), MIN("depth"), MAX("depth") FROM ({CLUSTERED}) '
        'GROUP BY "chrom", __giql_cluster_id ORDER BY "chrom", MIN("start")')


def sqlite_expected(rows, encoding):
    so, eo = OFFSETS[tuple(encoding)]
    conn = sqlite3.connect(":memory:")
    conn.execute("CREATE TABLE tgt (rid INTEGER, chrom TEXT, s INTEGER, e INTEGER)")
    conn.executemany("INSERT INTO tgt VALUES (?, ?, ?, ?)", [(i, r[0], r[1] + so, r[2] + eo) for i, r in enumerate(rows)])
    segments = [list(r) for r in conn.execute(SEGMENTS.format(so=so, eo=eo)).fetchall()]
    runs = None
    if encoding[1] == "half_open":
        conn.execute('CREATE TABLE segments (chrom TEXT, "start" INTEGER, "end" INTEGER, depth INTEGER)')
        conn.executemany("INSERT INTO segments VALUES (?, ?, ?, ?)", segments)
        runs = []
        for c, s, e, lo, hi in conn.execute(RUNS).fetchall():
            assert lo == hi, "a run shares one depth"
            runs.append([c, s, e, lo])
    conn.close()
    return segments, runs


def random_case(rng, k):
    encoding = list(list(OFFSETS)[k % 4])
    so, eo = OFFSETS[tuple(encoding)]
    chroms = [f"chr{c + 1}" for c in range(rng.randint(1, 4))]
    grid = rng.choice([5, 10, 25])           # coarse coordinates: touching rows and shared boundaries are common
    top = rng.choice([60, 200, 1000])
    rows = []
    for _ in range(rng.randint(1, 14)):
        s = rng.randrange(0, top, grid) if rng.random() < 0.8 else rng.randrange(0, top)
        shape = rng.random()
        e = s if shape < 0.12 else s + grid * rng.randint(1, 4) if shape < 0.7 else s + rng.randint(1, top // 2)
        rows.append([rng.choice(chroms), s, e])
    for _ in range(rng.randint(0, 4)):       # duplicates, nested rows and rows that start where another ends
        c, s, e = rng.choice(rows)
        pick = rng.random()
        rows.append([c, s, e] if pick < 0.4 else [c, s, s + (e - s) // 2] if pick < 0.7 else [c, e, e + grid])
    rows = [[c, s - so, e - eo] for c, s, e in rows]
    segments, runs = sqlite_expected(rows, encoding)
    return {"id": f"random-{k:03d}", "encoding": encoding, "rows": rows, "segments": segments, "runs": runs}


def main():
    assert sqlite3.sqlite_version_info >= (3, 25), "LEAD needs sqlite 3.25"
    rng = random.Random(20261021)
    cases = [random_case(rng, k) for k in range(60)]
    with open(os.path.join(HERE, "coverage.json"), "w") as f:
        json.dump({"sqlite": sqlite3.sqlite_version, "cases": cases}, f, separators=(",", ":"))
        f.write("\n")
    merged = sum(len(c["segments"]) - len(c["runs"]) for c in cases if c["runs"] is not None)
    print(len(cases), "cases,", sum(len(c["segments"]) for c in cases), "segments,", merged, "merged away in runs")


if __name__ == "__main__":
    main()
