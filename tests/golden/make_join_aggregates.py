#!/usr/bin/env python3
"""Mint tests/golden/join_aggregates.json: grouped aggregates over an INTERSECTS join in the map shape -- bedtools
``map -c 5 -o mean,count,max`` and "Overlap Statistics" of docs/recipes -- grouped by the left interval, by the
left ``name`` (duplicate keys) and by the left ``chrom``.  The rows are the rows sqlite3 computes from the plain SQL
the shape stands for: ``a [LEFT] JOIN b ON a.chrom = b.chrom AND a.start < b.end AND b.start < a.end ... GROUP BY``.

sqlite's aggregates follow the NULL rules of DuckDB, the reference's execution target: SUM / AVG / MIN / MAX of no
non-NULL value is NULL, COUNT(col) of none is 0, COUNT(*) counts the padded row of an unmatched left row.  Scores
are multiples of 1/4, so every sum and every mean of the data is exact in binary64 whatever the order.  The left
intervals are distinct: grouped by the interval, a group is one left row.

Needs only the standard library (no reference code is imported)."""
import json
import os
import random
import sqlite3

HERE = os.path.dirname(os.path.abspath(__file__))
COLS = ("chrom", "start", "end", "name", "strand", "score", "weight")
AGGS = [("COUNT", "*"), ("COUNT", "name"), ("COUNT", "score"), ("SUM", "score"), ("AVG", "score"), ("MIN", "score"),
        ("MAX", "score"), ("SUM", "weight")]
KEYS = {"interval": ("chrom", "start", "end"), "name": ("name",), "chrom": ("chrom",)}


def make_rows(seed: int, sizes, names, null_names: float):
    r = random.Random(seed)
    rows, seen = [], set()
    for chrom, n in sizes:
        while n:
            start = r.randrange(0, 3000, 5)
            end = start + r.randint(5, 120)
            if (chrom, start, end) in seen:
                continue
            seen.add((chrom, start, end))
            n -= 1
            name = None if r.random() < null_names else r.choice(names)
            score = None if r.random() < 0.45 else r.randint(-200, 1600) / 4
            weight = None if r.random() < 0.3 else r.randint(-20, 90)
            rows.append((chrom, start, end, name, r.choice("+-"), score, weight))
    r.shuffle(rows)
    return rows


def answer(a_rows, b_rows, join: str, keys, strand: bool):
    db = sqlite3.connect(":memory:")
    for t, rows in (("a", a_rows), ("b", b_rows)):
        db.execute(f'CREATE TABLE {t} (chrom TEXT, "start" INT, "end" INT, name TEXT, strand TEXT, score REAL, weight INT)')
        db.executemany(f"INSERT INTO {t} VALUES (?, ?, ?, ?, ?, ?, ?)", rows)
    key = ", ".join(f'a."{k}"' for k in keys)
    aggs = ", ".join("COUNT(*)" if c == "*" else f'{f}(b."{c}")' for f, c in AGGS)
    on = 'a.chrom = b.chrom AND a."start" < b."end" AND b."start" < a."end"' + (" AND a.strand = b.strand" if strand else "")
    sql = f"SELECT {key}, {aggs} FROM a {join} JOIN b ON {on} GROUP BY {key} ORDER BY {key}"
    return [list(r) for r in db.execute(sql)]


def main() -> None:
    a_rows = make_rows(20261001, (("chr1", 40), ("chr2", 30), ("chrX", 12), ("chrM", 3)), ["g1", "g2", "g3", "g4", "g5"], 0.1)
    b_rows = make_rows(20261002, (("chr1", 140), ("chr2", 90), ("chrX", 30), ("chrY", 9)), ["x", "y", "z"], 0.25)
    cases = []
    for join in ("INNER", "LEFT"):
        for kname, keys in KEYS.items():
            for strand in (False, True):
                rows = answer(a_rows, b_rows, join, keys, strand)
                cases.append({"name": f"{join.lower()}_{kname}{'_strand' if strand else ''}", "join": join,
                              "keys": list(keys), "strand": strand, "rows": rows})
    k = 3
    left = next(c for c in cases if c["name"] == "left_interval")["rows"]
    assert any(r[k] == 1 and r[k + 1] == 0 and r[k + 3] is None for r in left), "want an unmatched left row"
    assert any(r[k] > 1 and r[k + 2] == 0 and r[k + 3] is None for r in left), "want a row whose scores are all NULL"
    assert any(r[k] > 1 and 0 < r[k + 2] < r[k] for r in left), "want a row with some NULL scores"
    assert any(r[0] is None for r in next(c for c in cases if c["name"] == "left_name")["rows"]), "want a NULL name key"
    doc = {"columns": list(COLS), "aggregates": [list(a) for a in AGGS], "a": [list(r) for r in a_rows],
           "b": [list(r) for r in b_rows], "cases": cases}
    with open(os.path.join(HERE, "join_aggregates.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
