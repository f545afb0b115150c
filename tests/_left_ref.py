"""Expectations for the LEFT OUTER join tests, written by hand:

* a numpy restatement of the row ids -- the INNER pairs of ``oracle.pyoracle`` plus ``(r, -1)`` for every left row
  ``np.setdiff1d`` finds without a pair;
* a ``sqlite3`` runner for whole queries: the tables are loaded as they are (NULLs included) and a plain
  ``LEFT JOIN`` is run whose ON clause spells the spatial predicate out.

SQLite serves as the judge of SQL's three-valued logic over the padded rows, of the aggregates' NULL handling and of
NULLS FIRST / LAST; it knows nothing of the operators, so each test writes its query twice from one template --
``{P}`` is the GIQL predicate in one and its expansion (:data:`PREDICATES`) in the other.
"""

from __future__ import annotations

import sqlite3

import numpy as np

from oracle import pyoracle as ora

#: the spatial predicates over 0-based half-open rows with start < end, aliases a (left) and b (right):
#: GIQL text -> SQL text.  DISTANCE as src/giql/expanders/_distance.py defines it for such rows: 0 when the rows
#: overlap, else the gap + 1.
_DIST = ('(CASE WHEN a.start < b."end" AND a."end" > b.start THEN 0 '
         'WHEN a."end" <= b.start THEN b.start - a."end" + 1 ELSE a.start - b."end" + 1 END)')
PREDICATES = {
    "a.interval INTERSECTS b.interval": 'a.chrom = b.chrom AND a.start < b."end" AND a."end" > b.start',
    "a.interval CONTAINS b.interval": 'a.chrom = b.chrom AND a.start <= b.start AND a."end" >= b."end"',
    "a.interval WITHIN b.interval": 'a.chrom = b.chrom AND b.start <= a.start AND b."end" >= a."end"',
    "DISTANCE(a.interval, b.interval) <= 40": f"a.chrom = b.chrom AND {_DIST} <= 40",
}
INTERSECTS = "a.interval INTERSECTS b.interval"


def pad_ids(row_a, n_rows: int) -> np.ndarray:
    """Ascending ids of ``[0, n_rows)`` that ``row_a`` does not hold."""
    return np.setdiff1d(np.arange(n_rows, dtype=np.int64), np.asarray(row_a, np.int64))


def left_rows(a: ora.Side, b: ora.Side) -> np.ndarray:
    """``[k, 2]`` (row_a, row_b) of ``a LEFT JOIN b ON a INTERSECTS b``, sorted; row_b = -1 on a padded row."""
    ra, rb = ora.c_inner(a, b, "sweep")
    pad = pad_ids(ra, a.n)
    return sort_rows(np.concatenate([ra.astype(np.int64), pad]),
                     np.concatenate([rb.astype(np.int64), np.full(pad.size, -1, np.int64)]))


def sort_rows(ra, rb) -> np.ndarray:
    p = np.stack([np.asarray(ra, np.int64), np.asarray(rb, np.int64)], 1)
    return p[np.lexsort((p[:, 1], p[:, 0]))]


def sqlite_rows(tables: dict, sql: str) -> list:
    """Run ``sql`` over ``{name: pyarrow.Table}`` in an in-memory SQLite database; the rows as tuples, in the order
    SQLite returns them."""
    con = sqlite3.connect(":memory:")
    try:
        for name, t in tables.items():
            cols = ", ".join(f'"{c}"' for c in t.column_names)
            con.execute(f'CREATE TABLE "{name}" ({cols})')
            rows = list(zip(*[t.column(c).to_pylist() for c in t.column_names]))
            con.executemany(f'INSERT INTO "{name}" VALUES ({", ".join("?" * len(t.column_names))})', rows)
        return [tuple(r) for r in con.execute(sql).fetchall()]
    finally:
        con.close()


def giql_and_sql(template: str, predicate: str = INTERSECTS) -> tuple:
    """``(GIQL text, SQLite text)`` of one query template whose ``{P}`` stands for the spatial predicate."""
    return template.replace("{P}", predicate), template.replace("{P}", PREDICATES[predicate])


def bag(rows) -> list:
    """Rows as a sorted multiset; NULL sorts first, floats are rounded to 9 places (AVG)."""
    def key(r):
        return tuple((0, 0) if v is None else (1, v) for v in r)

    return sorted((tuple(round(v, 9) if isinstance(v, float) else v for v in r) for r in rows), key=key)


# ---------------------------------------------------------------------- the tables and queries of the execute() tests
def random_table(rng, n, chroms, tag):
    """A few hundred rows; ``name`` (string), ``score`` (int32) and ``big`` (int64) hold NULLs of their own."""
    import pyarrow as pa

    start = rng.integers(0, 3000, n)
    length = rng.integers(10, 200, n)
    null = lambda p: rng.random(n) < p  # noqa: E731
    return pa.table({
        "chrom": pa.array([chroms[i] for i in rng.integers(0, len(chroms), n)], pa.string()),
        "start": pa.array(start, pa.int32()),
        "end": pa.array(start + length, pa.int32()),
        "name": pa.array([f"{tag}{i % 97}" for i in range(n)], pa.string(), mask=null(0.15)),
        "score": pa.array(rng.integers(0, 12, n), pa.int32(), mask=null(0.2)),
        "big": pa.array(rng.integers(2 ** 40, 2 ** 41, n), pa.int64(), mask=null(0.1)),
    })


def make_tables() -> dict:
    """``{"peaks": ..., "genes": ...}``; chr9 holds left rows only: every one of them is padded."""
    rng = np.random.default_rng(2024)
    return {"peaks": random_table(rng, 300, ["chr1", "chr2", "chr3", "chr9"], "p"),
            "genes": random_table(rng, 220, ["chr1", "chr2", "chr3"], "g")}


COLS = "a.name, a.start, a.score, b.name AS b_name, b.start AS b_start, b.score AS b_score, b.big AS b_big"
FROM = "FROM peaks a LEFT JOIN genes b ON {P}"
CASES = {
    "loj": f"SELECT {COLS} {FROM}",
    "v": f"SELECT a.chrom, a.start, a.name {FROM} WHERE b.chrom IS NULL",
    "v_with_residuals": f"SELECT a.chrom, a.start, a.name {FROM} AND b.score > 5 WHERE a.score > 2 AND b.start IS NULL",
    "on_left_only": f"SELECT {COLS} {FROM} AND a.score > 5",
    "on_right_only": f"SELECT {COLS} {FROM} AND b.score > 5",
    "on_two_sided": f"SELECT {COLS} {FROM} AND a.score < b.score",
    "on_all_three": f"SELECT {COLS} {FROM} AND a.score > 2 AND b.score > 3 AND a.start < b.start",
    "where_left": f"SELECT {COLS} {FROM} WHERE a.score > 5",
    "where_right": f"SELECT {COLS} {FROM} WHERE b.score > 5",
    "where_name_is_null": f"SELECT {COLS} {FROM} WHERE b.name IS NULL",
    "where_name_is_not_null": f"SELECT {COLS} {FROM} WHERE b.name IS NOT NULL",
    "where_not": f"SELECT {COLS} {FROM} WHERE NOT (b.score > 5)",
    "where_or_mixed": f"SELECT {COLS} {FROM} WHERE b.score > 5 OR a.score < 3",
    "where_or_with_null_test": f"SELECT {COLS} {FROM} WHERE b.score IS NULL OR a.score < b.score",
    "where_string": f"SELECT {COLS} {FROM} WHERE b.name > 'g40' OR a.name = 'p3'",
    "on_and_where": f"SELECT {COLS} {FROM} AND a.score > 4 WHERE b.score IS NULL OR b.score < 9",
    "distinct": f"SELECT DISTINCT a.chrom, b.score AS b_score {FROM}",
    "group": f"SELECT a.chrom, COUNT(*) AS n, SUM(b.score) AS s, MIN(b.score) AS lo, MAX(b.big) AS hi, AVG(b.score) AS m "
             f"{FROM} GROUP BY a.chrom",
    "group_all_padded": f"SELECT a.chrom, COUNT(*) AS n, SUM(b.score) AS s {FROM} AND a.score > 100 GROUP BY a.chrom",
}
