#!/usr/bin/env python3
"""Mint tests/golden/merge_string_agg.json: STRING_AGG beside MERGE -- "Collect Feature Names" of
docs/recipes/clustering.rst, bedtools ``merge -c 4 -o collapse``.  The reference keeps a plain aggregate beside MERGE
and evaluates it under the per-cluster GROUP BY (src/giql/expanders/merge.py:317-390), so its rows are the rows
sqlite3 computes here from that shape with ``group_concat(name, sep)``: a window over a window for the cluster id
(src/giql/expanders/cluster.py:210-300), then GROUP BY chrom[, strand], id -- the clustering SQL of
make_merge_aggregates.py.

sqlite's group_concat follows the NULL rules of DuckDB's string_agg: NULLs are skipped, no non-NULL input gives NULL,
an empty string is a value.  Its order inside a group is not this backend's (ascending start, then row), so the
golden rows are compared as token multisets per region plus NULL-ness; no name contains the separator, so splitting
is exact.  Starts are distinct inside a chromosome.

Needs only the standard library (no reference code is imported)."""
import json
import os
import random
import sqlite3

HERE = os.path.dirname(os.path.abspath(__file__))
COLS = ("chrom", "start", "end", "strand", "name")
SEP = ","
NAMES = ("geneA", "b", "", "λ-phage", "遺伝子7", "exon_12", "ß", "tRNA-Ala", "x" * 40)


def make_rows(seed: int):
    r = random.Random(seed)
    rows = []
    for chrom, n in (("chr1", 18), ("chr2", 14), ("chrX", 8)):
        for start in sorted(r.sample(range(0, 1200, 5), n)):
            name = None if r.random() < 0.3 else r.choice(NAMES)
            rows.append((chrom, start, start + r.randint(5, 70), r.choice("+-"), name))
    r.shuffle(rows)
    assert all(SEP not in (row[4] or "") for row in rows)
    return rows


def merged(rows, distance: int, stranded: bool):
    db = sqlite3.connect(":memory:")
    db.execute('CREATE TABLE t (chrom TEXT, "start" INT, "end" INT, strand TEXT, name TEXT)')
    db.executemany("INSERT INTO t VALUES (?, ?, ?, ?, ?)", rows)
    part = "chrom, strand" if stranded else "chrom"
    sql = f"""
        WITH lag_calc AS (
          SELECT *, MAX("end") OVER (PARTITION BY {part} ORDER BY "start"
                                     ROWS BETWEEN UNBOUNDED PRECEDING AND 1 PRECEDING) AS prev_max FROM t),
        flagged AS (
          SELECT *, CASE WHEN prev_max + {distance} >= "start" THEN 0 ELSE 1 END AS is_new FROM lag_calc),
        clustered AS (
          SELECT *, SUM(is_new) OVER (PARTITION BY {part} ORDER BY "start") AS cid FROM flagged)
        SELECT {part}, MIN("start"), MAX("end"), COUNT(*), COUNT(name), group_concat(name, ?)
        FROM clustered GROUP BY {part}, cid ORDER BY chrom, MIN("start")"""
    return [list(r) for r in db.execute(sql, (SEP,))]


def main() -> None:
    rows = make_rows(20260202)
    assert any(r[4] == "" for r in rows) and any(r[4] and len(r[4].encode()) > len(r[4]) for r in rows)
    cases = []
    for name, distance, stranded in (("d0", 0, False), ("d25", 25, False), ("d25_stranded", 25, True)):
        out = merged(rows, distance, stranded)
        assert any(r[-2] == 0 and r[-1] is None for r in out), "want a region whose names are all NULL"
        assert any(0 < r[-2] < r[-3] for r in out), "want a region with some NULL names"
        cases.append({"name": name, "distance": distance, "stranded": stranded, "merged": out})
    doc = {"columns": list(COLS), "separator": SEP, "rows": [list(r) for r in rows], "cases": cases}
    with open(os.path.join(HERE, "merge_string_agg.json"), "w") as f:
        json.dump(doc, f, indent=1, ensure_ascii=False)
        f.write("\n")


if __name__ == "__main__":
    main()
