"""STRING_AGG beside MERGE restated in plain Python (``string_aggregates=True``; docs/recipes/clustering.rst
"Collect Feature Names", bedtools ``merge -c 4 -o collapse``).  The regions are ``_merge_agg_ref.regions``; inside a
region the members are ordered by (start, row of the input table) -- the order this backend promises where DuckDB
leaves it unspecified -- NULLs (``None``) are skipped, and a region with nothing left is ``None``.  An empty string is
a value: it brings its separator."""
import _merge_agg_ref as R


def string_agg(values, separator: str):
    """DuckDB's ``string_agg`` over values already in order (``None`` = NULL)."""
    vals = [v for v in values if v is not None]
    return separator.join(vals) if vals else None


def members_in_order(members, start):
    return sorted(members, key=lambda i: (int(start[i]), i))


def merge_string_agg(part, start, end, distance, columns, aggs, holds=None):
    """Rows ``[partition, MIN(start), MAX(end), COUNT(*), string, ...]`` ordered by (partition, start).
    ``columns``: name -> per-row values (``str`` / ``bytes`` / ``None``); ``aggs``: ``[(column name, separator)]``."""
    out = []
    for p, members in R.regions(part, start, end, distance, holds):
        rows = members_in_order(members, start)
        out.append([p, min(int(start[i]) for i in members), max(int(end[i]) for i in members), len(members)]
                   + [string_agg([columns[c][i] for i in rows], sep) for c, sep in aggs])
    return out
