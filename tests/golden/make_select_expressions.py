#!/usr/bin/env python3
"""Mint tests/golden/select_expressions.json: joins whose SELECT list computes a column -- bedtools' -wo / -wao
``overlap_bp`` of docs/recipes/bedtools-migration.rst and docs/recipes/intersect.rst, the same over CONTAINS, WITHIN
and ``DISTANCE(...) <= N``, a searched CASE on a string comparison, a float column in a product and a division.  The
reference hands such a SELECT item to its engine as SQL text, so its rows are the rows sqlite3 computes here from
the same expression text beside the spelt-out join predicate (three-valued logic included: ``score`` holds NULLs).

sqlite differs from DuckDB, the reference's execution target, in two places, and the queries below stay clear of both:

* ``/`` between two integers truncates in sqlite and is a floating division in DuckDB: the minting SQL -- and only
  it, never the GIQL text -- writes such a division with a floating operand (``* 1.0 /``);
* the scalar ``min`` / ``max`` standing for LEAST / GREATEST return NULL on a NULL argument where DuckDB skips it:
  LEAST / GREATEST only ever see the non-NULL ``start`` / ``end`` columns here.

Needs only the standard library (no reference code is imported)."""
import json
import os
import random
import sqlite3

HERE = os.path.dirname(os.path.abspath(__file__))
COLS = ("chrom", "start", "end", "name", "score", "strand", "weight")
OVERLAP_BP = "LEAST(a.end, b.end) - GREATEST(a.start, b.start)"
# DISTANCE of two half-open intervals on one chromosome (src/giql/expanders/_distance.py:67-117, the plain variant):
# 0 where they overlap, else the gap + 1
DISTANCE_SQL = ('CASE WHEN a."start" < b."end" AND a."end" > b."start" THEN 0 WHEN a."end" <= b."start" '
                'THEN b."start" - a."end" + 1 ELSE a."start" - b."end" + 1 END')
JOINS = {
    "intersects": ("a.interval INTERSECTS b.interval", 'a."start" < b."end" AND a."end" > b."start"'),
    "contains": ("a.interval CONTAINS b.interval", 'a."start" <= b."start" AND a."end" >= b."end"'),
    "within": ("a.interval WITHIN b.interval", 'a."start" >= b."start" AND a."end" <= b."end"'),
    "distance": ("DISTANCE(a.interval, b.interval) <= 40", f"({DISTANCE_SQL}) <= 40"),
}

# (id, join, LEFT?, [(alias, GIQL expression, sqlite expression or None = the same text)])
CASES = [
    ("wo", "intersects", False, [("overlap_bp", f"({OVERLAP_BP})", None)]),
    ("wao", "intersects", True, [("overlap_bp", f"CASE WHEN b.chrom IS NULL THEN 0 ELSE {OVERLAP_BP} END", None)]),
    # without the CASE a padded row yields NULL where plain arithmetic meets the right side (LEAST / GREATEST would
    # skip its NULLs in DuckDB and not in sqlite: they stay out of this one)
    ("left-plain-arithmetic", "intersects", True, [("d", "b.end - a.start", None), ("w", "a.end - a.start", None)]),
    ("wo-contains", "contains", False, [("overlap_bp", f"({OVERLAP_BP})", None)]),
    ("wo-within", "within", False, [("overlap_bp", f"({OVERLAP_BP})", None)]),
    ("wo-distance", "distance", False, [("overlap_bp", f"({OVERLAP_BP})", None)]),
    ("case-on-a-string", "intersects", False,
     [("v", "CASE WHEN b.strand = '+' THEN a.score + b.score WHEN a.score IS NULL THEN -1 WHEN a.name < b.name THEN 7 END", None)]),
    ("float-product", "intersects", False,
     [("w", f"a.weight * ({OVERLAP_BP})", None), ("half", "0.5 * (a.end - a.start) - b.weight", None)]),
    ("fraction", "intersects", False,
     [("frac", f"({OVERLAP_BP}) / (a.end - a.start)", f"({OVERLAP_BP}) * 1.0 / (a.end - a.start)"),
      ("per_score", "(b.end - b.start) / a.score", "(b.end - b.start) * 1.0 / a.score")]),      # NULL on a zero divisor in both
    ("left-case-chain", "intersects", True,
     [("k", "CASE WHEN b.score IS NULL THEN ABS(a.start - a.end) WHEN b.score > a.score THEN -b.score ELSE a.score * b.score END", None),
      ("n", "CASE WHEN b.strand = a.strand THEN 1 END", None)]),
]


def quote(text: str) -> str:
    for side in "ab":
        text = text.replace(f"{side}.start", f'{side}."start"').replace(f"{side}.end", f'{side}."end"')
    return text.replace("LEAST(", "min(").replace("GREATEST(", "max(").replace("ABS(", "abs(")


def giql_query(join: str, left: bool, items) -> str:
    cols = "a.name AS an, a.start AS s, b.name AS bn, b.end AS e, " + ", ".join(f"{g} AS {alias}" for alias, g, _ in items)
    if left:
        return f"SELECT {cols} FROM features_a a LEFT JOIN features_b b ON {JOINS[join][0]}"
    if join == "intersects":    # the WHERE-form cross join the recipes use
        return f"SELECT {cols} FROM features_a a, features_b b WHERE {JOINS[join][0]}"
    return f"SELECT {cols} FROM features_a a JOIN features_b b ON {JOINS[join][0]}"


def sqlite_rows(conn, join: str, left: bool, items):
    cols = 'a.name, a."start", b.name, b."end", ' + ", ".join(quote(s or g) for _alias, g, s in items)
    cond = f"a.chrom = b.chrom AND {JOINS[join][1]}"
    return conn.execute(f"SELECT {cols} FROM features_a a {'LEFT ' if left else ''}JOIN features_b b ON {cond}").fetchall()


# touching, nested, identical, far-apart and unmatched rows; NULL scores; a chromosome only one table has
FIXED_A = [("chr1", 100, 200, "a0", 3, "+", 0.5), ("chr1", 200, 300, "a1", None, "-", 1.25), ("chr1", 150, 160, "a2", 0, "+", 0.1),
           ("chr1", 1000, 1100, "a3", 5, "-", 2.0), ("chr2", 10, 500, "a4", 2, "+", -1.5), ("chr9", 5, 50, "a5", 1, "+", 3.0),
           ("chr2", 600, 700, "a6", None, "-", 0.75)]
FIXED_B = [("chr1", 100, 200, "b0", 2, "+", 0.25), ("chr1", 120, 180, "b1", None, "-", 1.5), ("chr1", 300, 400, "b2", 4, "+", 2.5),
           ("chr1", 190, 210, "b3", 0, "-", 0.1), ("chr2", 0, 1000, "b4", 3, "-", -0.5), ("chr2", 100, 110, "b5", 1, "+", 4.0),
           ("chr3", 5, 50, "b6", 1, "+", 1.0), ("chr2", 705, 720, "b7", 6, "+", 8.0)]


def rand_rows(rng, n, tag):
    out = []
    for i in range(n):
        s = rng.randrange(0, 1500)
        score = None if rng.random() < 0.2 else rng.randrange(0, 6)
        out.append((rng.choice(["chr1", "chr2", "chr3"]), s, s + rng.randrange(1, 300), f"{tag}{i % 11}", score,
                    rng.choice("+-"), rng.choice((0.1, 0.5, 1.25, -2.0, 3.0, 1e-3, 7.75))))
    return out


def main() -> None:
    rng = random.Random(20261019)
    cases = []
    for cid, join, left, items in CASES:
        for size in ("fixed", "random"):
            fa, fb = (FIXED_A, FIXED_B) if size == "fixed" else (rand_rows(rng, 50, "a"), rand_rows(rng, 40, "b"))
            conn = sqlite3.connect(":memory:")
            for t, rows in (("features_a", fa), ("features_b", fb)):
                conn.execute(f'CREATE TABLE {t} (chrom TEXT, "start" INTEGER, "end" INTEGER, name TEXT, score INTEGER, '
                             "strand TEXT, weight REAL)")
                conn.executemany(f"INSERT INTO {t} VALUES (?, ?, ?, ?, ?, ?, ?)", rows)
            got = sqlite_rows(conn, join, left, items)
            conn.close()
            key = lambda r: tuple((x is None, x) for x in r)
            cases.append({"id": f"{cid}-{size}", "join": join, "left": left, "query": giql_query(join, left, items),
                          "aliases": [alias for alias, _g, _s in items],
                          "features_a": [list(r) for r in fa], "features_b": [list(r) for r in fb],
                          "rows": [list(r) for r in sorted(got, key=key)]})
    assert all(c["rows"] for c in cases)
    assert any(r[2] is None for c in cases if c["left"] for r in c["rows"])           # unmatched rows under LEFT
    assert any(r[4] is not None and r[4] <= 0 for c in cases if c["join"] == "distance" for r in c["rows"])  # touching / apart
    doc = {"_source": "tests/golden/make_select_expressions.py: sqlite3 evaluates the spelt-out join and the SELECT-list "
                      "expression text; rows are (a.name, a.start, b.name, b.end, <the computed columns>), sorted with "
                      "NULLs last per column; table rows are (chrom, start, end, name, score, strand, weight)",
           "columns": list(COLS), "cases": cases}
    with open(os.path.join(HERE, "select_expressions.json"), "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    print(len(cases), "cases,", sum(len(c["rows"]) for c in cases), "rows")


if __name__ == "__main__":
    main()
