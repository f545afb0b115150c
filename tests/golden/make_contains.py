"""Mint tests/golden/contains_within.json: column-to-column CONTAINS / WITHIN joins with their expected pairs.
Standard library and sqlite3 only.

Two kinds of case:

* ``known``: the column-to-column answers the reference's own suite asserts
  (tests/integration/bedtools/test_contains.py:57-85, test_within.py:58-83), transcribed as data with their
  ``file:line``;
* ``random``: seeded cases whose expected pairs come from sqlite3 executing the predicate the reference emits
  (``_column_join``, src/giql/expanders/intersects.py:155-166), written out below in SQL of its own, on canonical
  0-based half-open coordinates.

A case: ``enc_a`` / ``enc_b`` (the tables' declared encodings), ``a`` / ``b`` as ``[chrom, start, end]`` rows in
their table's encoding, ``contains`` = sorted ``[row_a, row_b]`` with ``a.interval CONTAINS b.interval`` and
``within`` = the same for ``a.interval WITHIN b.interval``.  ``tags`` name what the case was drawn to cover.

The seeded cases are re-drawn until: every side has fewer than 200 rows, at most 10 % of them have an empty
``contains`` set, and at least half hold a pair that overlaps without being contained.

    python tests/golden/make_contains.py
"""

import json
import os
import random
import sqlite3

HERE = os.path.dirname(os.path.abspath(__file__))
OFFSETS = {("0based", "half_open"): (0, 0), ("0based", "closed"): (0, 1),
           ("1based", "half_open"): (-1, -1), ("1based", "closed"): (-1, 0)}
ENCODINGS = list(OFFSETS)

KNOWN = [  # (source, a rows, b rows, a CONTAINS b, a WITHIN b)
    ("tests/integration/bedtools/test_contains.py:57",
     [("chr1", 100, 400), ("chr1", 200, 250)], [("chr1", 150, 300), ("chr1", 210, 240)],
     [(0, 0), (0, 1), (1, 1)], None),
    ("tests/integration/bedtools/test_within.py:58",
     [("chr1", 150, 250), ("chr1", 50, 400)], [("chr1", 100, 300)],
     None, [(0, 0)]),
]

CONTAINS_SQL = ("SELECT a.rid, b.rid FROM a, b "
                "WHERE a.chrom = b.chrom AND a.s <= b.s AND a.e >= b.e ORDER BY 1, 2")
WITHIN_SQL = ("SELECT a.rid, b.rid FROM a, b "
              "WHERE a.chrom = b.chrom AND a.s >= b.s AND a.e <= b.e ORDER BY 1, 2")
OVERLAP_NOT_CONTAINED_SQL = ("SELECT COUNT(*) FROM a, b WHERE a.chrom = b.chrom AND a.s < b.e AND a.e > b.s "
                             "AND NOT (a.s <= b.s AND a.e >= b.e)")


def sqlite_expected(a, b, enc_a, enc_b):
    """(contains, within, overlapping-but-not-contained count); rows arrive in their declared encodings."""
    conn = sqlite3.connect(":memory:")
    for name, rows, enc in (("a", a, enc_a), ("b", b, enc_b)):
        so, eo = OFFSETS[tuple(enc)]
        conn.execute(f"CREATE TABLE {name} (rid INTEGER, chrom TEXT, s INTEGER, e INTEGER)")
        conn.executemany(f"INSERT INTO {name} VALUES (?, ?, ?, ?)",
                         [(i, r[0], r[1] + so, r[2] + eo) for i, r in enumerate(rows)])
    contains = [list(r) for r in conn.execute(CONTAINS_SQL).fetchall()]
    within = [list(r) for r in conn.execute(WITHIN_SQL).fetchall()]
    loose = conn.execute(OVERLAP_NOT_CONTAINED_SQL).fetchone()[0]
    conn.close()
    return contains, within, loose


def random_case(rng, k):
    enc_a, enc_b = ENCODINGS[k % 4], ENCODINGS[(k // 4) % 4]     # all 16 pairs within every 16 cases
    n_chrom = 1 + k % 4
    chroms = [f"chr{c + 1}" for c in range(n_chrom)]
    a_chroms, b_chroms = chroms, chroms
    tags = []
    if n_chrom > 1 and k % 3 == 0:      # a chromosome absent from one side
        if k % 2:
            a_chroms = chroms[:-1]
        else:
            b_chroms = chroms[1:]
        tags.append("absent-chrom")
    top = rng.choice([80, 400, 3000])
    uniform = {5: 1, 6: rng.choice([7, 20]), 7: 1}.get(k % 8)     # the inner side b has one length L
    irregular_a = k % 8 in (1, 3)
    irregular_b = k % 8 in (2, 3) and uniform is None
    # outer rows: canonical, some short (shorter than L when the inner side is uniform)
    a = []
    for _ in range(rng.randint(4, 40)):
        s = rng.randrange(0, top)
        ln = rng.choice([1, 2, 3, 5]) if rng.random() < 0.3 else rng.randint(4, max(5, top // 2))
        a.append([rng.choice(a_chroms), s, s + ln])
    b = []
    for _ in range(rng.randint(4, 40)):
        s = rng.randrange(0, top)
        b.append([rng.choice(b_chroms), s, s + (uniform or rng.randint(1, max(2, top // 6)))])
    # rows of b built from rows of a: identical, equal start, equal end, one position too long at either end
    for _ in range(rng.randint(3, 10)):
        c, s, e = rng.choice(a)
        if c not in b_chroms:
            continue
        if uniform:
            pick = rng.choice([(s, s + uniform), (e - uniform, e), (e - uniform + 1, e + 1), (s - 1, s - 1 + uniform)])
        else:
            mid = rng.randint(s, e - 1)
            pick = rng.choice([(s, e), (s, mid + 1), (mid, e), (s - 1, e), (s, e + 1), (s + 1, e), (mid, mid + 1)])
        if pick[0] >= 0:
            b.append([c, pick[0], pick[1]])
    if uniform:
        tags.append(f"uniform-inner-L{uniform}")
        if any(r[2] - r[1] < uniform for r in a):
            tags.append("outer-shorter-than-L")
    if irregular_a:
        for _ in range(rng.randint(1, 4)):
            c, s, e = rng.choice(a + [r for r in b if r[0] in a_chroms])
            point = rng.choice([s, e, rng.randint(min(s, e), max(s, e))])
            a.append([c, point, point] if rng.random() < 0.7 else [c, point + rng.randint(1, 9), point])
        tags.append("irregular-outer")
    if irregular_b:
        for _ in range(rng.randint(1, 4)):
            c, s, e = rng.choice(b + [r for r in a if r[0] in b_chroms])
            point = rng.choice([s, e, rng.randint(min(s, e), max(s, e))])
            b.append([c, point, point] if rng.random() < 0.7 else [c, point + rng.randint(1, 9), point])
        tags.append("irregular-inner")
    if irregular_a and irregular_b:     # an identical zero-length row on both sides: [p,p) CONTAINS [p,p)
        c = rng.choice([x for x in a_chroms if x in b_chroms])
        p = rng.randrange(0, top)
        a.append([c, p, p])
        b.append([c, p, p])
    rng.shuffle(a)
    rng.shuffle(b)
    # canonical -> the declared encodings
    (aso, aeo), (bso, beo) = OFFSETS[enc_a], OFFSETS[enc_b]
    a = [[c, s - aso, e - aeo] for c, s, e in a]
    b = [[c, s - bso, e - beo] for c, s, e in b]
    contains, within, loose = sqlite_expected(a, b, enc_a, enc_b)
    return {"id": f"random-{k:03d}", "enc_a": list(enc_a), "enc_b": list(enc_b), "a": a, "b": b, "tags": tags,
            "loose_overlaps": loose, "contains": contains, "within": within}


def main():
    cases = []
    for source, a, b, contains, within in KNOWN:
        a, b = [list(r) for r in a], [list(r) for r in b]
        enc = ("0based", "half_open")
        got_c, got_w, loose = sqlite_expected(a, b, enc, enc)
        if contains is not None:
            assert got_c == [list(p) for p in contains], source
        if within is not None:
            assert got_w == [list(p) for p in within], source
        cases.append({"id": "known-" + source.rsplit("/", 1)[1], "source": source, "enc_a": list(enc), "enc_b": list(enc),
                      "a": a, "b": b, "tags": ["known"], "loose_overlaps": loose, "contains": got_c, "within": got_w})
    seed = 20261017
    while True:       # re-draw until the conditions of the module docstring hold
        rng = random.Random(seed)
        drawn = [random_case(rng, k) for k in range(100)]
        small = all(len(c["a"]) < 200 and len(c["b"]) < 200 for c in drawn)
        empty = sum(not c["contains"] for c in drawn)
        loose = sum(c["loose_overlaps"] > 0 for c in drawn)
        if small and empty <= len(drawn) // 10 and 2 * loose >= len(drawn):
            break
        seed += 1
    cases += drawn
    with open(os.path.join(HERE, "contains_within.json"), "w") as f:
        json.dump({"sqlite": sqlite3.sqlite_version, "seed": seed, "cases": cases}, f, separators=(",", ":"))
        f.write("\n")
    print(len(cases), "cases, seed", seed, ",", sum(len(c["contains"]) for c in cases), "contains pairs,",
          sum(len(c["within"]) for c in cases), "within pairs,", empty, "empty,", loose, "with loose overlaps")


if __name__ == "__main__":
    main()
