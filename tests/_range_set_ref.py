"""A NumPy restatement of literal range predicates in SQL's three-valued logic, for the range-set tests.

A three-valued array is a pair ``(value, known)`` of boolean arrays; ``value`` is read only where ``known``.  One term
per range, ``chrom = c AND <cmp on start> AND <cmp on end>`` (src/giql/expanders/intersects.py:85-133), OR-ed for ANY
and AND-ed for ALL (243-270); a WHERE keeps the rows whose condition is known and true.  tests/test_range_sets.py
checks this file against tests/golden/range_sets.json (sqlite3's answers), the GPU tests check the kernel against it.
"""

import numpy as np

OFFSETS = {("0based", "half_open"): (0, 0), ("0based", "closed"): (0, 1),
           ("1based", "half_open"): (-1, -1), ("1based", "closed"): (-1, 0)}
COMPARE = {"intersects": (np.less, np.greater), "contains": (np.less_equal, np.greater_equal),
           "within": (np.greater_equal, np.less_equal)}


def and3(parts):
    """Kleene AND of ``[(value, known)]``: FALSE where a known part is false, else NULL where a part is unknown."""
    false = np.zeros_like(parts[0][0], dtype=bool)
    unknown = np.zeros_like(false)
    for value, known in parts:
        false |= known & ~value
        unknown |= ~known
    return ~false & ~unknown, false | ~unknown


def or3(parts):
    true = np.zeros_like(parts[0][0], dtype=bool)
    unknown = np.zeros_like(true)
    for value, known in parts:
        true |= known & value
        unknown |= ~known
    return true, true | ~unknown


def not3(part):
    return ~part[0], part[1]


def any_over_bounds(op, chrom, start, end, ok_chrom, ok_start, ok_end, set_chrom, on_start, on_end):
    """``(value, valid)`` uint8 arrays of ``HipEngine.range_set_any`` for one set: chromosome codes and raw columns
    (any integer dtype) with their validity (boolean arrays), the set as codes and the bounds the columns are
    compared with.  An empty table gives empty arrays."""
    cmp_s, cmp_e = COMPARE[op]
    start, end = np.asarray(start, np.int64), np.asarray(end, np.int64)
    terms = [and3([(np.asarray(chrom) == c, ok_chrom), (cmp_s(start, np.int64(bs)), ok_start),
                   (cmp_e(end, np.int64(be)), ok_end)])
             for c, bs, be in zip(set_chrom, on_start, on_end)]
    value, known = or3(terms)
    return (value & known).astype(np.uint8), known.astype(np.uint8)


def _columns(case):
    cols = case["columns"]
    n = len(cols["chrom"])
    so, eo = OFFSETS[tuple(case["encoding"])]
    ok_c = np.array([c is not None for c in cols["chrom"]], dtype=bool).reshape(n)
    ok_s = np.array([v is not None for v in cols["start"]], dtype=bool).reshape(n)
    ok_e = np.array([v is not None for v in cols["end"]], dtype=bool).reshape(n)
    chrom = np.array(["" if c is None else c for c in cols["chrom"]], dtype=object).reshape(n)
    start = np.array([0 if v is None else v + so for v in cols["start"]], dtype=np.int64).reshape(n)   # canonical
    end = np.array([0 if v is None else v + eo for v in cols["end"]], dtype=np.int64).reshape(n)
    return chrom, start, end, ok_c, ok_s, ok_e


def predicate(pred, case):
    """One predicate of a golden case over the case's table -> ``(value, known)``, the NOT applied."""
    chrom, start, end, ok_c, ok_s, ok_e = _columns(case)
    cmp_s, cmp_e = COMPARE[pred["op"]]
    terms = []
    for c, lo, hi in pred["ranges"]:
        on_start, on_end = (hi, lo) if pred["op"] == "intersects" else (lo, hi)
        terms.append(and3([(chrom == c, ok_c), (cmp_s(start, on_start), ok_s), (cmp_e(end, on_end), ok_e)]))
    out = or3(terms) if pred["quantifier"] == "any" else and3(terms)
    return not3(out) if pred["negated"] else out


def kept_rows(case):
    """The ascending row ids a golden case's WHERE keeps."""
    parts = [predicate(p, case) for p in case["predicates"]]
    if case["compare"]:
        column, op, value = case["compare"]
        assert op == ">="
        vals = case["columns"][column]
        known = np.array([v is not None for v in vals], dtype=bool)
        parts.append((np.array([0 if v is None else v for v in vals]) >= value, known))
    value, known = and3(parts)
    return np.flatnonzero(value & known).tolist()
