"""The fixed list of queries of tests/test_coverage.py: the coverage profile of one table through DISJOIN, inside and
outside what the ``disjoin_aggregates`` opt-in lowers.  ``tests/golden/coverage_plans.json`` holds what every one of
them lowered to -- a plan string or the error -- WITHOUT the flag at the commit the file names
(tests/golden/make_coverage_plans.py recorded it from that commit's package)."""

from giql_amd.table import Table

#: "features", "other": 0-based half-open; "closed1": 1-based closed; "closed0": 0-based closed; "open1": 1-based half-open
TABLES = [Table("features"), Table("other"), Table("closed1", coordinate_system="1based", interval_type="closed"),
          Table("closed0", interval_type="closed"), Table("open1", coordinate_system="1based")]

KEYS = "disjoin_chrom, disjoin_start, disjoin_end"
SEG = "disjoin_chrom AS chrom, disjoin_start AS start, disjoin_end AS end"
DEPTH = f"SELECT {SEG}, COUNT(*) AS depth FROM DISJOIN(features) GROUP BY {KEYS}"
RUNS = f"SELECT MERGE(interval, predicate := depth = PREV(depth)) FROM ({DEPTH}) AS segments"

#: name -> (query, the ``segments`` of the plan it lowers to with the flag)
ACCEPTED = {
    "depth_recipe": (DEPTH, "depth"),
    "depth_plain_names": (f"SELECT {KEYS}, COUNT(*) AS n FROM DISJOIN(features) GROUP BY {KEYS}", "depth"),
    "depth_keys_reordered": (f"SELECT {SEG}, COUNT(*) AS depth FROM DISJOIN(features) "
                             "GROUP BY disjoin_end, disjoin_chrom, disjoin_start", "depth"),
    "depth_alias_qualified": (f"SELECT d.disjoin_start AS s, COUNT(*) AS depth FROM DISJOIN(features) AS d "
                              "GROUP BY d.disjoin_chrom, d.disjoin_start, d.disjoin_end", "depth"),
    "depth_two_counts": (f"SELECT COUNT(*) AS a, {KEYS}, COUNT(*) AS b FROM DISJOIN(features) d GROUP BY {KEYS}", "depth"),
    "depth_count_only": (f"SELECT COUNT(*) AS depth FROM DISJOIN(features) GROUP BY {KEYS}", "depth"),
    "depth_order_limit": (DEPTH + " ORDER BY depth DESC, chrom, start LIMIT 3 OFFSET 1", "depth"),
    "depth_order_hidden_key": (f"SELECT disjoin_start, COUNT(*) AS depth FROM DISJOIN(features) GROUP BY {KEYS} "
                               "ORDER BY disjoin_end DESC", "depth"),
    "depth_closed_target": (DEPTH.replace("features", "closed1"), "depth"),
    "distinct_recipe": (f"SELECT DISTINCT {KEYS} FROM DISJOIN(features)", "distinct"),
    "distinct_reordered_aliased": ("SELECT DISTINCT disjoin_end AS e, disjoin_chrom, disjoin_start AS s "
                                   "FROM DISJOIN(closed0) ORDER BY s LIMIT 5", "distinct"),
    "runs_recipe": (RUNS, "runs"),
    "runs_operands_swapped": (RUNS.replace("depth = PREV(depth)", "PREV(depth) = depth"), "runs"),
    "runs_other_count_alias": (RUNS.replace("depth", "n"), "runs"),
    "runs_no_alias": (RUNS.replace(" AS segments", ""), "runs"),
    "runs_bare_alias_qualified": (RUNS.replace("MERGE(interval", "MERGE(s.interval").replace(" AS segments", " s"), "runs"),
    "runs_order_limit": (RUNS + " ORDER BY chrom DESC, start LIMIT 4", "runs"),
    "runs_one_based_half_open": (RUNS.replace("features", "open1"), "runs"),
}

#: name -> (query, a fragment of the reason it declines with under the flag)
DECLINED = {
    "count_without_alias": (f"SELECT {KEYS}, COUNT(*) FROM DISJOIN(features) GROUP BY {KEYS}", "COUNT(*) without an alias"),
    "count_of_column": (f"SELECT {KEYS}, COUNT(name) AS n FROM DISJOIN(features) GROUP BY {KEYS}", "COUNT(name)"),
    "other_aggregate": (f"SELECT {KEYS}, SUM(score) AS s FROM DISJOIN(features) GROUP BY {KEYS}", "SUM("),
    "count_distinct": (f"SELECT {KEYS}, COUNT(DISTINCT name) AS n FROM DISJOIN(features) GROUP BY {KEYS}", "COUNT(DISTINCT"),
    "target_column": (f"SELECT {KEYS}, name, COUNT(*) AS n FROM DISJOIN(features) GROUP BY {KEYS}", "target column 'name'"),
    "star": (f"SELECT *, COUNT(*) AS n FROM DISJOIN(features) GROUP BY {KEYS}", "star projection"),
    "two_keys": ("SELECT disjoin_chrom, COUNT(*) AS n FROM DISJOIN(features) GROUP BY disjoin_chrom, disjoin_start",
                 "other than exactly"),
    "four_keys": (f"SELECT {KEYS}, COUNT(*) AS n FROM DISJOIN(features) GROUP BY {KEYS}, name", "other than exactly"),
    "key_twice": ("SELECT COUNT(*) AS n FROM DISJOIN(features) GROUP BY disjoin_chrom, disjoin_start, disjoin_start",
                  "other than exactly"),
    "reference_mode": (DEPTH.replace("DISJOIN(features)", "DISJOIN(features, reference := other)"), "reference :="),
    "where": (DEPTH.replace(" GROUP BY", " WHERE disjoin_start > 5 GROUP BY"), "WHERE over the rows of DISJOIN"),
    "having": (DEPTH + " HAVING COUNT(*) > 1", "HAVING over the rows of DISJOIN"),
    "aggregate_without_group_by": ("SELECT COUNT(*) AS n FROM DISJOIN(features)", "GROUP BY / aggregates over the rows"),
    "distinct_and_group_by": (DEPTH.replace("SELECT ", "SELECT DISTINCT ", 1), "DISTINCT beside GROUP BY"),
    "order_by_target_column": (DEPTH + " ORDER BY name", "ORDER BY 'name'"),
    "runs_distance": (RUNS.replace("MERGE(interval,", "MERGE(interval, 10,"), "MERGE distance"),
    "runs_stranded": (RUNS.replace("MERGE(interval,", "MERGE(interval, stranded := true,"), "stranded"),
    "runs_other_predicate": (RUNS.replace("depth = PREV(depth)", "depth >= PREV(depth)"), "predicate other than"),
    "runs_two_conjuncts": (RUNS.replace("depth = PREV(depth)", "depth = PREV(depth) AND depth = 2"), "predicate other than"),
    "runs_predicate_on_start": (RUNS.replace("depth = PREV(depth)", "start = PREV(start)"), "predicate other than"),
    "runs_no_predicate": (RUNS.replace(", predicate := depth = PREV(depth)", ""), "predicate other than"),
    "runs_count_beside": (RUNS.replace("PREV(depth))", "PREV(depth)), COUNT(*) AS n"), "aggregate beside MERGE"),
    "runs_column_beside": (RUNS.replace("SELECT MERGE", "SELECT chrom, MERGE", 1), "column beside MERGE"),
    "runs_cluster": (RUNS.replace("SELECT MERGE(interval, predicate := depth = PREV(depth))",
                                  "SELECT *, CLUSTER(interval) AS c"), "CLUSTER over a sub-query"),
    "runs_plain_subquery": ("SELECT MERGE(interval) FROM (SELECT chrom, start, end FROM features) AS t", "other than the coverage"),
    "runs_ungrouped_disjoin": (f"SELECT MERGE(interval) FROM (SELECT {SEG} FROM DISJOIN(features)) AS t", "other than the coverage"),
    "runs_unnamed_columns": (RUNS.replace(SEG, KEYS), "as chrom, start, end"),
    "runs_inner_limit": (RUNS.replace(f"GROUP BY {KEYS}", f"GROUP BY {KEYS} LIMIT 5"), "inside the coverage sub-query"),
    "runs_outer_where": (RUNS + " WHERE start > 3", "WHERE clause with MERGE"),
    "runs_closed_target": (RUNS.replace("features", "closed1"), "closed-interval target"),
    "runs_closed_zero_based": (RUNS.replace("features", "closed0"), "closed-interval target"),
}

#: name -> query: with the flag they lower, decline or fail exactly as without it
OUTSIDE = {
    "distinct_two_columns": "SELECT DISTINCT disjoin_chrom, disjoin_start FROM DISJOIN(features)",
    "distinct_with_target_column": f"SELECT DISTINCT {KEYS}, name FROM DISJOIN(features)",
    "distinct_reference_mode": f"SELECT DISTINCT {KEYS} FROM DISJOIN(features, reference := other)",
    "ungrouped_three": f"SELECT {KEYS} FROM DISJOIN(features)",
    "star": "SELECT * FROM DISJOIN(features) ORDER BY disjoin_start LIMIT 2",
    "merge_on_table": "SELECT MERGE(interval), COUNT(*) AS n FROM features",
    "cluster_predicate_on_table": "SELECT *, CLUSTER(interval, predicate := score = PREV(score)) AS c FROM features",
}


def all_queries() -> dict:
    out = {f"accepted/{k}": q for k, (q, _s) in ACCEPTED.items()}
    out.update({f"declined/{k}": q for k, (q, _r) in DECLINED.items()})
    out.update({f"outside/{k}": q for k, q in OUTSIDE.items()})
    return out


def outcome(build_plan, query: str, **opts) -> dict:
    """What ``build_plan`` makes of a query: ``{"plan": <string form>}`` or ``{"error": <class name>, "message": ...}``."""
    try:
        return {"plan": build_plan(query, TABLES, **opts).to_string()}
    except ValueError as exc:       # (HipDeclined is one)
        return {"error": type(exc).__name__, "message": str(exc)}
