"""Mint tests/golden/distance.json: DISTANCE values and within-distance pair sets.  Standard library and sqlite3
only; run HERE only (the reference tree does not travel).

Two kinds of case:

* ``known``: the answers the reference's own suite asserts for DISTANCE (tests/test_distance_udf.py), transcribed as
  data with their ``file:line``: one A row, one B row, the variant (``stranded`` / ``signed``) and the expected value
  (``null`` = SQL NULL).  Each is ALSO checked against sqlite3 below before it is written;
* ``random``: seeded cases -- at most 64 x 64 rows on 3 chromosomes, the four coordinate encodings in turn, strands
  drawn from ``+ - . ?`` and NULL, zero-length rows, book-ended rows, rows repeated across chromosomes -- whose
  expected values come from stdlib ``sqlite3`` executing the text of the reference's own ``generate_distance_case``
  (src/giql/expanders/_distance.py:22-117; sqlglot-free, loaded BY FILE PATH at generation time) over the cartesian
  product of the two tables, on canonical 0-based half-open coordinates (src/giql/canonical.py:16-52 applied as
  ``start + start_off`` / ``end + end_off``).

A random case holds ``enc_a`` / ``enc_b``, ``a`` / ``b`` as ``[chrom, start, end, strand | null]`` rows in their
table's encoding, and

* ``pairs``: ``[row_a, row_b]`` of every same-chromosome pair, sorted;
* ``values``: per variant ``"plain" | "signed" | "stranded" | "stranded_signed"`` the value of every pair of ``pairs``
  (``null`` = SQL NULL; cross-chromosome pairs are NULL in every variant and not listed);
* ``within``: per N in {0, 1, 2, 50, 2^40} the sorted ``[row_a, row_b]`` with ``DISTANCE(a, b) <= N`` -- the recipe
  of docs/recipes/distance.rst:60-73, sqlite3 filtering the plain CASE.

    python tests/golden/make_distance.py
"""

import importlib.util
import json
import os
import random
import sqlite3

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OFFSETS = {("0based", "half_open"): (0, 0), ("0based", "closed"): (0, 1),
           ("1based", "half_open"): (-1, -1), ("1based", "closed"): (-1, 0)}
ENCODINGS = list(OFFSETS)
WITHIN_N = [0, 1, 2, 50, 1 << 40]
VARIANTS = {"plain": (False, False), "signed": (False, True), "stranded": (True, False),
            "stranded_signed": (True, True)}

U = "tests/test_distance_udf.py"
KNOWN = [  # (source, a row, b row, variant, expected)
    (f"{U}:94", ("chr1", 100, 200, None), ("chr1", 300, 400, None), "plain", 101),
    (f"{U}:118", ("chr1", 100, 200, None), ("chr2", 150, 250, None), "plain", None),
    (f"{U}:145", ("chr1", 100, 200, None), ("chr1", 200, 300, None), "plain", 1),
    (f"{U}:169", ("chr1", 150, 150, None), ("chr1", 300, 400, None), "plain", 151),
    (f"{U}:193", ("chr1", 100, 200, None), ("chr1", 201, 300, None), "plain", 2),
    (f"{U}:240", ("chr1", 100, 200, None), ("chr1", 199, 300, None), "plain", 0),
    (f"{U}:260", ("chr1", 300, 400, None), ("chr1", 100, 200, None), "plain", 101),
    (f"{U}:284", ("chr1", 100, 200, None), ("chr1", 200, 300, None), "signed", 1),
    (f"{U}:305", ("chr1", 200, 300, None), ("chr1", 100, 200, None), "signed", -1),
    (f"{U}:330", ("chr1", 100, 200, "+"), ("chr1", 300, 400, "+"), "stranded", 101),
    (f"{U}:353", ("chr1", 100, 200, "-"), ("chr1", 300, 400, "-"), "stranded", -101),
    (f"{U}:376", ("chr1", 100, 200, "+"), ("chr1", 300, 400, "-"), "stranded", 101),
    (f"{U}:399", ("chr1", 100, 200, "-"), ("chr1", 300, 400, "+"), "stranded", -101),
    (f"{U}:422", ("chr1", 100, 200, "."), ("chr1", 300, 400, "."), "stranded", None),
    (f"{U}:447", ("chr1", 100, 200, "?"), ("chr1", 300, 400, "+"), "stranded", None),
    (f"{U}:472", ("chr1", 100, 200, None), ("chr1", 300, 400, "+"), "stranded", None),
    (f"{U}:497", ("chr1", 100, 200, "-"), ("chr1", 150, 250, "-"), "stranded", 0),
    (f"{U}:524", ("chr1", 100, 200, "+"), ("chr1", 200, 300, "+"), "stranded", 1),
    (f"{U}:545", ("chr1", 100, 200, "-"), ("chr1", 200, 300, "-"), "stranded", -1),
    (f"{U}:566", ("chr1", 300, 400, "+"), ("chr1", 100, 200, "+"), "stranded", 101),
    (f"{U}:586", ("chr1", 300, 400, "-"), ("chr1", 100, 200, "-"), "stranded", -101),
    (f"{U}:630", ("chr1", 300, 400, "+"), ("chr1", 100, 200, "+"), "stranded_signed", -101),
    (f"{U}:651", ("chr1", 300, 400, "-"), ("chr1", 100, 200, "-"), "stranded_signed", 101),
    (f"{U}:672", ("chr1", 100, 200, "-"), ("chr1", 200, 300, "-"), "stranded_signed", -1),
    (f"{U}:694", ("chr1", 100, 200, "."), ("chr1", 200, 300, "+"), "stranded_signed", None),
]


def _load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_DIST = _load_by_path("_ref_distance", os.path.join(REF, "src", "giql", "expanders", "_distance.py"))


def case_sql(variant):
    stranded, signed = VARIANTS[variant]
    return _DIST.generate_distance_case("a.chrom", "a.s", "a.e", "a.strand" if stranded else None,
                                        "b.chrom", "b.s", "b.e", "b.strand" if stranded else None,
                                        stranded=stranded, signed=signed)


def connect(a, b, enc_a, enc_b):
    conn = sqlite3.connect(":memory:")
    for name, rows, enc in (("a", a, enc_a), ("b", b, enc_b)):
        so, eo = OFFSETS[tuple(enc)]
        conn.execute(f"CREATE TABLE {name} (rid INTEGER, chrom TEXT, s INTEGER, e INTEGER, strand TEXT)")
        conn.executemany(f"INSERT INTO {name} VALUES (?, ?, ?, ?, ?)",
                         [(i, r[0], r[1] + so, r[2] + eo, r[3]) for i, r in enumerate(rows)])
    return conn


def expected(a, b, enc_a, enc_b):
    conn = connect(a, b, enc_a, enc_b)
    pairs = [list(r) for r in conn.execute(
        "SELECT a.rid, b.rid FROM a, b WHERE a.chrom = b.chrom ORDER BY 1, 2").fetchall()]
    values = {}
    for variant in VARIANTS:
        values[variant] = [r[0] for r in conn.execute(
            f"SELECT {case_sql(variant)} FROM a, b WHERE a.chrom = b.chrom ORDER BY a.rid, b.rid").fetchall()]
        cross = conn.execute(f"SELECT COUNT(*) FROM a, b WHERE a.chrom != b.chrom AND ({case_sql(variant)}) IS NOT NULL")
        assert cross.fetchone()[0] == 0
    within = {}
    for n in WITHIN_N:
        within[str(n)] = [list(r) for r in conn.execute(
            f"SELECT a.rid, b.rid FROM a, b WHERE a.chrom = b.chrom AND ({case_sql('plain')}) <= {n} ORDER BY 1, 2").fetchall()]
    conn.close()
    return pairs, values, within


def random_case(rng, k):
    enc_a, enc_b = ENCODINGS[k % 4], ENCODINGS[(k + 1 + k // 4) % 4]
    chroms = ["chr1", "chr2", "chr3"]
    a_chroms = chroms[:-1] if k % 3 == 1 else chroms          # a chromosome present on one side only
    b_chroms = chroms[1:] if k % 3 == 2 else chroms
    top = rng.choice([60, 300, 5000])
    strands = ["+", "-", ".", "?", None]

    def rows(n, names):
        out = []
        for _ in range(n):
            s = rng.randrange(0, top)
            ln = 0 if rng.random() < 0.15 else rng.randint(1, max(2, top // 8))     # zero-length rows too
            out.append([rng.choice(names), s, s + ln, rng.choice(strands)])
        return out

    a = rows(rng.randint(8, 28), a_chroms)
    b = rows(rng.randint(8, 18), b_chroms)
    # rows of b placed against rows of a: book-ended on either end, 1 / 2 / 50 / 51 positions away, identical,
    # and the same coordinates on ANOTHER chromosome
    shared = [r for r in a if r[0] in b_chroms]
    for j, gap in enumerate([0, 1, 2, 49, 50, 51, 0, 1, 0, 50]):
        c, s, e, _st = rng.choice(shared)
        ln = rng.randint(0, 9)
        pick = (e + gap, e + gap + ln) if j % 2 == 0 or s - gap - ln < 0 else (s - gap - ln, s - gap)
        if j == 5:
            pick = (s, e)
        cc = rng.choice([x for x in b_chroms if x != c]) if j >= 8 else c      # the last two: another chromosome
        b.append([cc, pick[0], pick[1], rng.choice(strands)])
    rng.shuffle(a)
    rng.shuffle(b)
    (aso, aeo), (bso, beo) = OFFSETS[enc_a], OFFSETS[enc_b]
    a = [[c, s - aso, e - aeo, st] for c, s, e, st in a]       # canonical -> the declared encodings
    b = [[c, s - bso, e - beo, st] for c, s, e, st in b]
    pairs, values, within = expected(a, b, enc_a, enc_b)
    return {"id": f"random-{k:02d}", "enc_a": list(enc_a), "enc_b": list(enc_b), "a": a, "b": b,
            "pairs": pairs, "values": values, "within": within}


def main():
    known = []
    enc = ("0based", "half_open")
    for source, ra, rb, variant, want in KNOWN:
        _pairs, values, _within = expected([list(ra)], [list(rb)], enc, enc)
        got = values[variant][0] if ra[0] == rb[0] else None
        assert got == want, (source, got, want)
        known.append({"id": "known-" + source.rsplit("/", 1)[1], "source": source, "a": list(ra), "b": list(rb),
                      "variant": variant, "expected": want})
    seed = 20261018
    while True:       # re-draw until every case covers what it was drawn to cover
        rng = random.Random(seed)
        drawn = [random_case(rng, k) for k in range(6)]
        ok = all(len(c["a"]) <= 64 and len(c["b"]) <= 64 for c in drawn)
        # book-ended pairs: out at N = 0, in at N = 1; 2^40 takes every same-chromosome pair
        ok = ok and all(c["within"]["0"] and len(c["within"]["1"]) > len(c["within"]["0"]) for c in drawn)
        ok = ok and all(len(c["within"][str(1 << 40)]) == len(c["pairs"]) for c in drawn)
        for v in ("stranded", "stranded_signed"):   # NULLs and flipped signs in every case
            ok = ok and all(any(x is None for x in c["values"][v]) and any(x is not None and x < 0 for x in c["values"][v])
                            for c in drawn)
        if ok:
            break
        seed += 1
    path = os.path.join(HERE, "distance.json")
    with open(path, "w") as f:
        json.dump({"sqlite": sqlite3.sqlite_version, "seed": seed, "within_n": WITHIN_N, "known": known,
                   "random": drawn}, f, separators=(",", ":"))
        f.write("\n")
    print(len(known), "known,", len(drawn), "random cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
