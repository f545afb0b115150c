"""Aggregates of per-pair expressions over a join's pairs per left row, restated on the host: the value of a tree at a
pair comes from tests/_expr_ref.py (a negative id is the NULL row of its side), the reduction per left row from
tests/_pair_agg_ref.py (``aggregate``: exact, in ascending ``row_b``).  No torch, no HIP library.

The value an aggregate sees follows the static type rule of the computed columns: where ``_expr_ref.can_float`` says
the tree can yield a float every value is ``float(value)`` (an integer value is rounded once), otherwise it is the
Python integer; ``None`` is SQL NULL and is no input of the aggregate."""
import numpy as np

import _expr_ref as E
import _pair_agg_ref as R


def pair_values(tree, row_a, row_b):
    """The tree's value per pair ``(row_a[i], row_b[i])``, typed as the aggregate sees it."""
    vals = E.values(tree, [int(x) for x in row_a], [int(x) for x in row_b])
    if E.can_float(tree):
        return [None if v is None else float(E._int(v)) for v in vals]
    return [None if v is None else int(v) for v in vals]


def pair_expr_aggregate(row_a, row_b, n_a: int, aggs):
    """``(pairs, results, inputs)``: ``aggs`` is ``[(func, source)]`` with ``source`` a tree of tests/_expr_ref.py or
    ``("col", values)`` -- per-B-row Python values, ``None`` = NULL.  ``results[j][a]`` is the value for A row ``a``
    (``None`` = NULL; AVG is ``float(sum) / count``), ``inputs[j][a]`` the row's per-pair values in ascending
    ``row_b`` (what an error bound is scaled by)."""
    row_a, row_b = np.asarray(row_a, np.int64), np.asarray(row_b, np.int64)
    order = np.lexsort((row_b, row_a))
    sa, sb = row_a[order].tolist(), row_b[order].tolist()
    pairs = np.bincount(row_a, minlength=n_a).tolist() if len(row_a) else [0] * n_a
    results, inputs, memo = [], [], {}
    for func, source in aggs:
        if id(source) not in memo:
            vals = [source[1][b] for b in sb] if source[0] == "col" else pair_values(source, sa, sb)
            rows = [[] for _ in range(n_a)]
            for a, v in zip(sa, vals):
                rows[a].append(v)
            memo[id(source)] = rows
        rows = memo[id(source)]
        results.append([R.aggregate(func, r) for r in rows])
        inputs.append(rows)
    return pairs, results, inputs


def intersecting_pairs(a, b):
    """Brute force: the pairs ``(i, j)`` with equal chrom and ``a.start < b.end and a.end > b.start`` (half-open), of
    two tables given as dicts of Python lists with ``chrom`` / ``start`` / ``end``.  NULL coordinates match nothing."""
    out = []
    for i, (ca, sa, ea) in enumerate(zip(a["chrom"], a["start"], a["end"])):
        for j, (cb, sb, eb) in enumerate(zip(b["chrom"], b["start"], b["end"])):
            if None in (ca, sa, ea, cb, sb, eb):
                continue
            if ca == cb and sa < eb and ea > sb:
                out.append((i, j))
    return out


def query_rows(a, b, join: str, keys, aggs, trees):
    """The rows of ``SELECT <keys>, COUNT(*), <aggs> FROM a <join> JOIN b ON a INTERSECTS b GROUP BY <keys> ORDER BY
    <keys>`` by brute force: the pairs of ``intersecting_pairs``, under LEFT one padded row (right id -1, the NULL row)
    per left row without a pair; ``aggs`` is ``[(func, tree name)]``, ``trees`` maps a name to a tree over numpy
    columns of ``a`` / ``b``.  NULL keys sort first, as sqlite's."""
    pairs = intersecting_pairs(a, b)
    if join == "LEFT":
        matched = {i for i, _j in pairs}
        pairs += [(i, -1) for i in range(len(a["chrom"])) if i not in matched]
    pairs.sort()
    ra, rb = [p[0] for p in pairs], [p[1] for p in pairs]
    values = {name: pair_values(tree, ra, rb) for name, tree in trees.items()}
    groups = {}
    for pos, i in enumerate(ra):
        groups.setdefault(tuple(a[k][i] for k in keys), []).append(pos)
    rows = []
    for key in sorted(groups, key=lambda t: tuple((v is not None, v) for v in t)):
        at = groups[key]
        rows.append(list(key) + [len(at)] + [R.aggregate(f, [values[name][p] for p in at]) for f, name in aggs])
    return rows


def golden_tables(doc):
    """The two tables of tests/golden/aggregate_expressions.json as dicts of Python lists (``None`` = NULL)."""
    return tuple({c: [r[i] for r in doc[t]] for i, c in enumerate(doc["columns"])} for t in ("a", "b"))


def golden_trees(a, b):
    """The golden's five expressions (its ``expressions`` entry, by name) as trees over numpy columns of the tables."""
    def leaf(side, table, name):
        vals = table[name]
        valid = np.array([v is not None for v in vals])
        if name in ("chrom", "name"):
            data = np.zeros(len(vals), np.uint8)           # read for its validity alone
        else:
            data = np.array([0 if v is None else v for v in vals], np.float64 if name == "score" else np.int64)
        return (side, data, valid)

    overlap = ("-", ("least", leaf("a", a, "end"), leaf("b", b, "end")),
               ("greatest", leaf("a", a, "start"), leaf("b", b, "start")))
    return {
        "overlap_bp": overlap,
        "overlap_case": ("if", ("isnull", leaf("b", b, "chrom")), ("lit", 0), overlap),
        "weighted": ("*", leaf("b", b, "score"), overlap),
        "reach": ("-", leaf("b", b, "end"), leaf("a", a, "start")),
        "ratio": ("/", leaf("b", b, "score"), leaf("b", b, "weight")),
    }
