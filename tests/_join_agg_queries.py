"""The fixed list of queries of tests/test_join_aggregates.py: grouped aggregates over a join, inside and outside the
map shape of the ``join_aggregates`` opt-in.  ``tests/golden/join_aggregates_plans.json`` holds what every one of them
lowered to -- a plan string or the error -- WITHOUT the flag at the commit the file names
(tests/golden/make_join_aggregates_plans.py recorded it from that commit's package)."""

TABLES = ["a", "b"]
IV = "a.chrom, a.start, a.end"
ON = "a.interval INTERSECTS b.interval"

#: name -> query; in the map shape: with the flag they lower to a plan marked ``join_aggregates``
MAP_SHAPE = {
    # bedtools map -c 5 -o mean,count,max
    "left_count_avg_max": f"SELECT {IV}, AVG(b.score) AS mean, COUNT(b.score) AS n, MAX(b.score) AS mx "
                          f"FROM a LEFT JOIN b ON {ON} GROUP BY {IV}",
    "left_sum_only": f"SELECT a.name, SUM(b.score) AS s FROM a LEFT JOIN b ON {ON} GROUP BY a.name",
    "left_outer_count_star": f"SELECT {IV}, COUNT(*) AS rows_, MIN(b.weight) AS lo FROM a LEFT OUTER JOIN b ON {ON} GROUP BY {IV}",
    "left_lone_count_with_residual": f"SELECT {IV}, COUNT(b.name) AS n FROM a LEFT JOIN b ON {ON} AND a.strand = b.strand "
                                     f"GROUP BY {IV}",
    "inner_tail": f"SELECT a.name, SUM(b.score) AS s, COUNT(*) AS c FROM a JOIN b ON {ON} WHERE a.strand = b.strand "
                  "GROUP BY a.name HAVING COUNT(*) > 1 ORDER BY s DESC LIMIT 3",
    "inner_chrom_key": f"SELECT a.chrom, AVG(b.score) AS m, COUNT(b.name) AS n FROM a, b WHERE {ON} GROUP BY a.chrom",
    "inner_hidden_key": f"SELECT MAX(b.weight) AS hi FROM a JOIN b ON {ON} GROUP BY a.name",
    "inner_hidden_having": f"SELECT a.name, SUM(b.weight) AS w FROM a JOIN b ON {ON} GROUP BY a.name HAVING MIN(b.score) < 10",
    "inner_distinct": f"SELECT DISTINCT a.chrom, COUNT(*) AS c FROM a JOIN b ON {ON} GROUP BY a.chrom",
    "inner_contains": f"SELECT {IV}, SUM(b.score) AS s FROM a JOIN b ON a.interval CONTAINS b.interval GROUP BY {IV}",
    "left_within": f"SELECT {IV}, SUM(b.score) AS s, COUNT(b.name) AS n FROM a LEFT JOIN b ON a.interval WITHIN b.interval GROUP BY {IV}",
    "inner_distance": f"SELECT {IV}, MIN(b.score) AS lo FROM a JOIN b ON DISTANCE(a.interval, b.interval) <= 100 GROUP BY {IV}",
    "eight_aggregates": f"SELECT a.name, COUNT(*) AS c0, COUNT(b.name) AS c1, SUM(b.score) AS c2, AVG(b.score) AS c3, "
                        f"MIN(b.score) AS c4, MAX(b.score) AS c5, SUM(b.weight) AS c6, AVG(b.weight) AS c7 "
                        f"FROM a JOIN b ON {ON} GROUP BY a.name",
}

#: name -> query; outside the shape: with the flag they lower, decline or fail exactly as without it
OUTSIDE = {
    "lone_count_bare_on": f"SELECT {IV}, COUNT(b.name) AS n FROM a LEFT JOIN b ON {ON} GROUP BY {IV}",
    "right_side_key": f"SELECT b.name, SUM(b.score) AS s FROM a JOIN b ON {ON} GROUP BY b.name",
    "left_right_side_key": f"SELECT b.name, COUNT(b.score) AS n, SUM(b.score) AS s FROM a LEFT JOIN b ON {ON} GROUP BY b.name",
    "aggregate_of_left_column": f"SELECT a.name, SUM(a.score) AS s FROM a JOIN b ON {ON} GROUP BY a.name",
    "count_distinct": f"SELECT a.name, COUNT(DISTINCT b.name) AS n FROM a JOIN b ON {ON} GROUP BY a.name",
    "nine_aggregates": f"SELECT a.name, COUNT(*) AS c0, COUNT(b.name) AS c1, SUM(b.score) AS c2, AVG(b.score) AS c3, "
                       f"MIN(b.score) AS c4, MAX(b.score) AS c5, SUM(b.weight) AS c6, AVG(b.weight) AS c7, "
                       f"MAX(b.weight) AS c8 FROM a JOIN b ON {ON} GROUP BY a.name",
    "ninth_in_having": f"SELECT a.name, COUNT(*) AS c0, COUNT(b.name) AS c1, SUM(b.score) AS c2, AVG(b.score) AS c3, "
                       f"MIN(b.score) AS c4, MAX(b.score) AS c5, SUM(b.weight) AS c6, AVG(b.weight) AS c7 "
                       f"FROM a JOIN b ON {ON} GROUP BY a.name HAVING MAX(b.weight) > 3",
    "no_group_by": f"SELECT COUNT(*) AS c, SUM(b.score) AS s FROM a JOIN b ON {ON}",
    "unaliased_aggregate": f"SELECT a.name, SUM(b.score) FROM a JOIN b ON {ON} GROUP BY a.name",
    "left_unaliased_beside_count": f"SELECT a.name, COUNT(b.name) AS n, SUM(b.score) FROM a LEFT JOIN b ON {ON} GROUP BY a.name",
    "left_with_where": f"SELECT a.name, SUM(b.score) AS s FROM a LEFT JOIN b ON {ON} WHERE a.score > 3 GROUP BY a.name",
    "left_predicate_in_where": f"SELECT a.name, SUM(b.score) AS s FROM a LEFT JOIN b ON a.strand = b.strand WHERE {ON} GROUP BY a.name",
    "plain_column_not_a_key": f"SELECT a.name, a.score, SUM(b.score) AS s FROM a JOIN b ON {ON} GROUP BY a.name",
    "left_plain_column_not_a_key": f"SELECT a.name, a.score, COUNT(b.name) AS n, SUM(b.score) AS s FROM a LEFT JOIN b ON {ON} GROUP BY a.name",
    "having_over_left_column": f"SELECT a.name, SUM(b.score) AS s FROM a JOIN b ON {ON} GROUP BY a.name HAVING SUM(a.score) > 1",
    "semi_join": f"SELECT a.name, COUNT(*) AS c FROM a SEMI JOIN b ON {ON} GROUP BY a.name",
    "unqualified_key": f"SELECT a.name, SUM(b.score) AS s FROM a JOIN b ON {ON} GROUP BY name",
    "ungrouped_pairs": f"SELECT a.name, b.score FROM a JOIN b ON {ON}",
}

#: the opt-ins every query is lowered under (the flag itself apart)
OPTIONS = {"plain": {}, "outer_joins": {"outer_joins": True}}


def outcome(build_plan, query: str, **opts) -> dict:
    """What ``build_plan`` makes of a query: ``{"plan": <string form>}`` or ``{"error": <class name>, "message": ...}``."""
    try:
        return {"plan": build_plan(query, TABLES, **opts).to_string()}
    except ValueError as exc:       # (HipDeclined is one)
        return {"error": type(exc).__name__, "message": str(exc)}
