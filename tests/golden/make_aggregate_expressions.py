#!/usr/bin/env python3
"""Mint tests/golden/aggregate_expressions.json: aggregates of per-pair EXPRESSIONS over an INTERSECTS join in the map
shape -- "Overlap Statistics" of docs/recipes/advanced.rst and what `bedtools intersect -wo | groupby` computes --
grouped by the left interval, by the left ``name`` (duplicate keys) and by the left ``chrom``, INNER and LEFT.  The
rows are the rows sqlite3 computes from the plain SQL the shape stands for.

The expressions: overlap_bp (``LEAST(a.end, b.end) - GREATEST(a.start, b.start)``), its ``CASE WHEN b.chrom IS NULL
THEN 0 ELSE ... END`` form, ``b.score * overlap_bp``, ``b.end - a.start`` and ``b.score / b.weight``.  sqlite has no
NULL-skipping LEAST / GREATEST (its MIN(x, y) is NULL when an argument is): they are written as a CASE that skips a
NULL argument, which is DuckDB's rule, the reference's execution target; ``/`` is written as a division of REALs
(NULL on a zero divisor in both).  Scores are multiples of 1/4 and the weights 0 or plus / minus a power of two up to
4, so every value is a multiple of 1/16 and every sum of the data is exact in binary64 whatever the order.

Under LEFT an unmatched left row is one padded row: overlap_bp of it is ``a.end - a.start`` (both right arguments are
skipped), the CASE form gives 0, the other three are NULL.

Needs only the standard library (no reference code is imported)."""
import json
import os
import random
import sqlite3

HERE = os.path.dirname(os.path.abspath(__file__))
COLS = ("chrom", "start", "end", "name", "score", "weight")
FUNCS = ("COUNT", "SUM", "AVG", "MIN", "MAX")
KEYS = {"interval": ("chrom", "start", "end"), "name": ("name",), "chrom": ("chrom",)}


def least(x, y):
    return f"(CASE WHEN {x} IS NULL THEN {y} WHEN {y} IS NULL THEN {x} WHEN {x} < {y} THEN {x} ELSE {y} END)"


def greatest(x, y):
    return f"(CASE WHEN {x} IS NULL THEN {y} WHEN {y} IS NULL THEN {x} WHEN {x} > {y} THEN {x} ELSE {y} END)"


OVERLAP = "(" + least('a."end"', 'b."end"') + " - " + greatest('a."start"', 'b."start"') + ")"
#: name -> (the GIQL text of the expression, the sqlite text)
EXPRESSIONS = {
    "overlap_bp": ("LEAST(a.end, b.end) - GREATEST(a.start, b.start)", OVERLAP),
    "overlap_case": ("CASE WHEN b.chrom IS NULL THEN 0 ELSE LEAST(a.end, b.end) - GREATEST(a.start, b.start) END",
                     f"(CASE WHEN b.chrom IS NULL THEN 0 ELSE {OVERLAP} END)"),
    "weighted": ("b.score * (LEAST(a.end, b.end) - GREATEST(a.start, b.start))", f"(b.score * {OVERLAP})"),
    "reach": ("b.end - a.start", '(b."end" - a."start")'),
    "ratio": ("b.score / b.weight", "(CAST(b.score AS REAL) / CAST(b.weight AS REAL))"),
}


def make_rows(seed: int, sizes, names, null_names: float):
    r = random.Random(seed)
    rows, seen = [], set()
    for chrom, n in sizes:
        while n:
            start = r.randrange(0, 2000, 5)
            end = start + r.randint(5, 120)
            if (chrom, start, end) in seen:
                continue
            seen.add((chrom, start, end))
            n -= 1
            name = None if r.random() < null_names else r.choice(names)
            score = None if r.random() < 0.4 else r.randint(-200, 1600) / 4
            weight = None if r.random() < 0.2 else r.choice([0, 1, 2, 4, -1, -2])
            rows.append((chrom, start, end, name, score, weight))
    r.shuffle(rows)
    return rows


def answer(a_rows, b_rows, join: str, keys):
    db = sqlite3.connect(":memory:")
    for t, rows in (("a", a_rows), ("b", b_rows)):
        db.execute(f'CREATE TABLE {t} (chrom TEXT, "start" INT, "end" INT, name TEXT, score REAL, weight INT)')
        db.executemany(f"INSERT INTO {t} VALUES (?, ?, ?, ?, ?, ?)", rows)
    key = ", ".join(f'a."{k}"' for k in keys)
    aggs = ", ".join(f"{f}({sql})" for _giql, sql in EXPRESSIONS.values() for f in FUNCS)
    on = 'a.chrom = b.chrom AND a."start" < b."end" AND b."start" < a."end"'
    sql = f"SELECT {key}, COUNT(*), {aggs} FROM a {join} JOIN b ON {on} GROUP BY {key} ORDER BY {key}"
    return [list(r) for r in db.execute(sql)]


def main() -> None:
    a_rows = make_rows(20261101, (("chr1", 18), ("chr2", 12), ("chrX", 5), ("chrM", 2)), ["g1", "g2", "g3", "g4"], 0.1)
    b_rows = make_rows(20261102, (("chr1", 50), ("chr2", 30), ("chrX", 10), ("chrY", 4)), ["x", "y"], 0.25)
    cases = []
    for join in ("INNER", "LEFT"):
        for kname, keys in KEYS.items():
            cases.append({"name": f"{join.lower()}_{kname}", "join": join, "keys": list(keys),
                          "rows": answer(a_rows, b_rows, join, keys)})
    # the cases the file exists for, in the LEFT rows keyed by the (distinct) interval: the columns after the key are
    # COUNT(*), then COUNT / SUM / AVG / MIN / MAX per expression in the order of EXPRESSIONS
    k, n = 3, len(FUNCS)
    col = {name: k + 1 + j * n for j, name in enumerate(EXPRESSIONS)}
    left = next(c for c in cases if c["name"] == "left_interval")["rows"]
    unmatched = [r for r in left if r[k] == 1 and r[col["reach"]] == 0]
    assert unmatched and all(r[col["overlap_bp"] + 1] == r[2] - r[1] for r in unmatched), \
        "an unmatched left row sums overlap_bp to a.end - a.start"
    assert all(r[col["overlap_case"]] == 1 and r[col["overlap_case"] + 1] == 0 for r in unmatched), "... and to 0 under the CASE"
    assert all(r[col["reach"] + 1] is None and r[col["weighted"] + 1] is None for r in unmatched), "... and to NULL otherwise"
    assert any(r[col["reach"]] >= 1 and r[col["weighted"]] == 0 and r[col["weighted"] + 1] is None for r in left), \
        "want a matched row whose values are all NULL"
    assert any(r[k] > 1 and 0 < r[col["ratio"]] < r[k] for r in left), "want a row with some NULL ratios (a zero divisor)"
    assert any(r[0] is None for r in next(c for c in cases if c["name"] == "left_name")["rows"]), "want a NULL name key"
    lines = ["{", f' "columns": {json.dumps(list(COLS))},', f' "functions": {json.dumps(list(FUNCS))},',
             f' "expressions": {json.dumps({n_: g for n_, (g, _s) in EXPRESSIONS.items()})},']
    for t, rows in (("a", a_rows), ("b", b_rows)):
        lines.append(f' "{t}": [\n' + ",\n".join("  " + json.dumps(list(r)) for r in rows) + "\n ],")
    lines.append(' "cases": [')
    for i, c in enumerate(cases):
        head = json.dumps({"name": c["name"], "join": c["join"], "keys": c["keys"]})[:-1]
        body = ",\n".join("   " + json.dumps(r, separators=(",", ":")) for r in c["rows"])
        lines.append(f'  {head}, "rows": [\n{body}\n  ]}}' + ("," if i + 1 < len(cases) else ""))
    lines += [" ]", "}"]
    text = "\n".join(lines) + "\n"
    json.loads(text)
    with open(os.path.join(HERE, "aggregate_expressions.json"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
