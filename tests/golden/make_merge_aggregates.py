#!/usr/bin/env python3
"""Mint tests/golden/merge_aggregates.json: MERGE with aggregates beside it -- ``merge -c 5 -o mean`` of
docs/recipes/bedtools-migration.rst and "Merge with Aggregations" of docs/recipes/clustering.rst.  The reference
keeps a plain aggregate beside MERGE and evaluates it under the per-cluster GROUP BY
(src/giql/expanders/merge.py:317-390), so its rows are the rows sqlite3 computes here from that shape: a window
over a window for the cluster id (src/giql/expanders/cluster.py:210-300), then GROUP BY chrom[, strand], id.

sqlite's aggregates follow the NULL rules of DuckDB, the reference's execution target: SUM / AVG / MIN / MAX of no
non-NULL value is NULL, COUNT(col) of none is 0.  sqlite has no NaN, so the data holds none.  Starts are distinct
inside a chromosome: the ROWS frame of the running maximum then has one order.

Needs only the standard library (no reference code is imported)."""
import json
import os
import random
import sqlite3

HERE = os.path.dirname(os.path.abspath(__file__))
COLS = ("chrom", "start", "end", "strand", "score", "weight")
AGGS = [(f, c) for c in ("score", "weight") for f in ("COUNT", "SUM", "AVG", "MIN", "MAX")]


def make_rows(seed: int):
    r = random.Random(seed)
    rows = []
    for chrom, n in (("chr1", 18), ("chr2", 14), ("chrX", 8)):
        for start in sorted(r.sample(range(0, 1200, 5), n)):
            score = None if r.random() < 0.3 else round(r.uniform(-50, 400), r.choice((0, 1, 2)))
            if score is not None:
                score = float(f"{score:.3g}")  # 3 significant digits
            weight = None if r.random() < 0.3 else r.randint(-20, 90)
            rows.append((chrom, start, start + r.randint(5, 70), r.choice("+-"), score, weight))
    r.shuffle(rows)
    return rows


def merged(rows, distance: int, stranded: bool):
    db = sqlite3.connect(":memory:")
    db.execute('CREATE TABLE t (chrom TEXT, "start" INT, "end" INT, strand TEXT, score REAL, weight INT)')
    db.executemany("INSERT INTO t VALUES (?, ?, ?, ?, ?, ?)", rows)
    part = "chrom, strand" if stranded else "chrom"
    aggs = ", ".join(f"{f}({c})" for f, c in AGGS)
    sql = f"""
        WITH lag_calc AS (
          SELECT *, MAX("end") OVER (PARTITION BY {part} ORDER BY "start"
                                     ROWS BETWEEN UNBOUNDED PRECEDING AND 1 PRECEDING) AS prev_max FROM t),
        flagged AS (
          SELECT *, CASE WHEN prev_max + {distance} >= "start" THEN 0 ELSE 1 END AS is_new FROM lag_calc),
        clustered AS (
          SELECT *, SUM(is_new) OVER (PARTITION BY {part} ORDER BY "start") AS cid FROM flagged)
        SELECT {part}, MIN("start"), MAX("end"), COUNT(*), {aggs}
        FROM clustered GROUP BY {part}, cid ORDER BY chrom, MIN("start")"""
    return [list(r) for r in db.execute(sql)]


def main() -> None:
    rows = make_rows(20260101)
    cases = []
    for name, distance, stranded in (("d0", 0, False), ("d25", 25, False), ("d25_stranded", 25, True)):
        out = merged(rows, distance, stranded)
        k = 5 if stranded else 4   # first aggregate column
        assert any(r[k] == 0 and r[k + 1] is None for r in out), "want a region whose scores are all NULL"
        assert any(r[k - 1] > 1 and r[k] not in (0, r[k - 1]) for r in out), "want a region with some NULL scores"
        cases.append({"name": name, "distance": distance, "stranded": stranded, "merged": out})
    doc = {"columns": list(COLS), "aggregates": [list(a) for a in AGGS], "rows": [list(r) for r in rows], "cases": cases}
    with open(os.path.join(HERE, "merge_aggregates.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
