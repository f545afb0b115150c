"""Mint tests/golden/disjoin.json: DISJOIN cases with their expected rows.  Standard library only.

Two kinds of case:

* ``known``: the ten answers the reference's own suite asserts (tests/test_disjoin_udf.py:63-290),
  transcribed as data with their ``file:line``;
* ``random``: seeded cases whose expected rows come from sqlite3 (>= 3.25 for LEAD) executing the CTE
  pipeline the reference emits for the case (src/giql/expanders/disjoin.py:147-202: breakpoints =
  UNION of the reference's starts and ends, cuts strictly inside a target, LEAD gaps, the EXISTS
  coverage filter unless the reference is the target), on canonical 0-based half-open coordinates,
  with the pieces moved back into the target's declared encoding (:136-140).

A case: ``encoding`` (of the target), ``target`` / ``reference`` (``null`` = self mode) as
``[chrom, start, end, name]`` rows in their table's encoding (the reference is always 0-based
half-open), ``expected`` as sorted ``[target row, disjoin_start, disjoin_end]``.  No row has
start > end: the backend rejects those.

    python tests/golden/make_disjoin.py
"""

import json
import os
import random
import sqlite3

HERE = os.path.dirname(os.path.abspath(__file__))
OFFSETS = {("0based", "half_open"): (0, 0), ("0based", "closed"): (0, 1),
           ("1based", "half_open"): (-1, -1), ("1based", "closed"): (-1, 0)}

KNOWN = [  # (tests/test_disjoin_udf.py line, target, reference, expected)
    (63, [("chr1", 0, 20, "A"), ("chr1", 10, 30, "B")], None, [(0, 0, 10), (0, 10, 20), (1, 10, 20), (1, 20, 30)]),
    (89, [("chr1", 0, 20, "A"), ("chr1", 10, 30, "B")], None, [(0, 0, 10), (0, 10, 20), (1, 10, 20), (1, 20, 30)]),
    (110, [("chr1", 0, 30, "T")], [("chr1", 0, 10, "a"), ("chr1", 10, 30, "b")], [(0, 0, 10), (0, 10, 30)]),
    (132, [("chr1", 0, 30, "T")], [("chr1", 0, 10, "a"), ("chr1", 20, 30, "b")], [(0, 0, 10), (0, 20, 30)]),
    (154, [("chr1", 5, 5, "P")], None, []),
    (174, [("chr1", 0, 10, "X"), ("chr1", 0, 10, "Y")], [("chr1", 0, 5, "a"), ("chr1", 5, 10, "b")],
     [(0, 0, 5), (0, 5, 10), (1, 0, 5), (1, 5, 10)]),
    (196, [("chr1", 0, 20, "A"), ("chr2", 5, 25, "B")], None, [(0, 0, 20), (1, 5, 25)]),
    (218, [("chr1", 0, 20, "A"), ("chr1", 10, 30, "B")], None, [(0, 0, 10), (0, 10, 20), (1, 10, 20), (1, 20, 30)]),
    (245, [("chr1", 0, 20, "T")], [("chr1", 0, 10, "bin0"), ("chr1", 10, 20, "bin1")], [(0, 0, 10), (0, 10, 20)]),
    (270, [("chr1", 10, 20, "T")], [("chr1", 10, 20, "r")], [(0, 10, 20)]),
]

PIPELINE = """
WITH __giql_dj_ref AS (SELECT * FROM {ref}), __giql_dj_tgt AS (SELECT * FROM tgt),
__giql_dj_bp AS (SELECT chrom, s AS pos FROM __giql_dj_ref UNION SELECT chrom, e AS pos FROM __giql_dj_ref),
__giql_dj_cuts AS (
  SELECT t.chrom AS kc, t.s AS ks, t.e AS ke, t.s AS pos FROM __giql_dj_tgt AS t
  UNION SELECT t.chrom AS kc, t.s AS ks, t.e AS ke, t.e AS pos FROM __giql_dj_tgt AS t
  UNION SELECT t.chrom AS kc, t.s AS ks, t.e AS ke, bp.pos AS pos FROM __giql_dj_tgt AS t
        JOIN __giql_dj_bp AS bp ON bp.chrom = t.chrom AND bp.pos > t.s AND bp.pos < t.e),
__giql_dj_segs AS (SELECT kc, ks, ke, pos AS seg_start,
                          LEAD(pos) OVER (PARTITION BY kc, ks, ke ORDER BY pos) AS seg_end FROM __giql_dj_cuts)
SELECT t.rid, s.seg_start, s.seg_end FROM __giql_dj_tgt AS t
JOIN __giql_dj_segs AS s ON t.chrom = s.kc AND t.s = s.ks AND t.e = s.ke
WHERE s.seg_end IS NOT NULL AND s.seg_end > s.seg_start{coverage}
"""
COVERAGE = (" AND EXISTS (SELECT 1 FROM __giql_dj_ref AS r WHERE r.chrom = s.kc "
            "AND r.s <= s.seg_start AND r.e > s.seg_start)")


def sqlite_expected(target, reference, encoding):
    """Rows of the emitted pipeline; target rows arrive in ``encoding``, the reference canonical."""
    so, eo = OFFSETS[tuple(encoding)]
    conn = sqlite3.connect(":memory:")
    conn.execute("CREATE TABLE tgt (rid INTEGER, chrom TEXT, s INTEGER, e INTEGER)")
    conn.executemany("INSERT INTO tgt VALUES (?, ?, ?, ?)",
                     [(i, r[0], r[1] + so, r[2] + eo) for i, r in enumerate(target)])
    if reference is not None:
        conn.execute("CREATE TABLE ref (chrom TEXT, s INTEGER, e INTEGER)")
        conn.executemany("INSERT INTO ref VALUES (?, ?, ?)", [(r[0], r[1], r[2]) for r in reference])
    sql = PIPELINE.format(ref="tgt" if reference is None else "ref", coverage="" if reference is None else COVERAGE)
    rows = conn.execute(sql).fetchall()
    conn.close()
    return sorted([rid, s - so, e - eo] for rid, s, e in rows)


def random_case(rng, k):
    encoding = list(list(OFFSETS)[k % 4])
    so, eo = OFFSETS[tuple(encoding)]
    chroms = [f"chr{c + 1}" for c in range(rng.randint(1, 4))]
    grid = rng.choice([5, 10, 25])           # coarse coordinates: touching rows and shared boundaries are common
    top = rng.choice([60, 200, 1000])

    def row(cs, allow_point, tag):
        s = rng.randrange(0, top, grid) if rng.random() < 0.7 else rng.randrange(0, top)
        shape = rng.random()
        if allow_point and shape < 0.12:
            e = s
        elif shape < 0.6:
            e = s + grid * rng.randint(1, 4)
        else:
            e = s + rng.randint(1, top // 2)
        return [rng.choice(cs), s, e, tag]

    self_mode = k % 3 == 0
    t_chroms = chroms if rng.random() < 0.6 else chroms[: max(1, len(chroms) - 1)]
    r_chroms = chroms if rng.random() < 0.6 else chroms[1:] or chroms   # chromosomes on one side only
    target = [row(t_chroms, True, f"t{i}") for i in range(rng.randint(1, 12))]
    for _ in range(rng.randint(0, 3)):       # duplicates and nested rows
        src = rng.choice(target)
        target.append(list(src[:3]) + [f"t{len(target)}"] if rng.random() < 0.5
                      else [src[0], src[1], src[1] + max(0, (src[2] - src[1]) // 2), f"t{len(target)}"])
    reference = None
    if not self_mode:
        reference = [row(r_chroms, True, f"r{i}") for i in range(rng.randint(0 if k % 11 == 1 else 1, 10))]
        if target and rng.random() < 0.5:    # a breakpoint exactly on a target boundary
            t = rng.choice(target)
            reference.append([t[0], t[1], t[2], "edge"])
        if rng.random() < 0.3:               # every target uncovered: the reference lies beyond them
            reference = [[r[0], r[1] + 10 * top, r[2] + 10 * top, r[3]] for r in reference]
    # canonical -> the target's declared encoding
    target = [[c, s - so, e - eo, n] for c, s, e, n in target]
    return {"id": f"random-{k:03d}", "encoding": encoding, "target": target, "reference": reference,
            "expected": sqlite_expected(target, reference, encoding)}


def main():
    assert sqlite3.sqlite_version_info >= (3, 25), "LEAD needs sqlite 3.25"
    cases = []
    for line, target, reference, expected in KNOWN:
        target = [list(r) for r in target]
        reference = [list(r) for r in reference] if reference is not None else None
        want = sorted(list(e) for e in expected)
        assert sqlite_expected(target, reference, ("0based", "half_open")) == want, line
        cases.append({"id": f"known-{line}", "source": f"tests/test_disjoin_udf.py:{line}",
                      "encoding": ["0based", "half_open"], "target": target, "reference": reference, "expected": want})
    rng = random.Random(20260117)
    cases += [random_case(rng, k) for k in range(100)]
    with open(os.path.join(HERE, "disjoin.json"), "w") as f:
        json.dump({"sqlite": sqlite3.sqlite_version, "cases": cases}, f, separators=(",", ":"))
        f.write("\n")
    print(len(cases), "cases,", sum(len(c["expected"]) for c in cases), "expected rows")


if __name__ == "__main__":
    main()
