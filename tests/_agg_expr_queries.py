"""The fixed list of queries of tests/test_aggregate_expressions.py: aggregates over an EXPRESSION of a join's pair,
inside the map shape of the ``join_aggregates`` + ``aggregate_expressions`` opt-ins, the ones that decline with them,
and neighbours that never held such an aggregate.  ``tests/golden/aggregate_expressions_plans.json`` holds what every
one of them lowered to -- a plan string or the error -- at the commit the file names, which is BEFORE the
``aggregate_expressions`` opt-in existed, under each set of the other opt-ins
(tests/golden/make_aggregate_expressions_plans.py recorded it from that commit's package)."""

TABLES = ["a", "b"]
IV = "a.chrom, a.start, a.end"
ON = "a.interval INTERSECTS b.interval"
OV = "LEAST(a.end, b.end) - GREATEST(a.start, b.start)"
CASE = f"CASE WHEN b.chrom IS NULL THEN 0 ELSE {OV} END"

#: name -> query; with both opt-ins they lower to a map-shape plan whose aggregates of side "x" name expressions
IN_SHAPE = {
    # "Overlap Statistics", docs/recipes/advanced.rst
    "overlap_statistics": f"SELECT a.chrom, COUNT(*) AS overlap_count, AVG({OV}) AS avg_overlap_bp, "
                          f"SUM({OV}) AS total_overlap_bp FROM a INNER JOIN b ON {ON} GROUP BY a.chrom ORDER BY a.chrom",
    "left_covered_bp": f"SELECT {IV}, SUM({OV}) AS bp FROM a LEFT JOIN b ON {ON} GROUP BY {IV}",
    "left_case": f"SELECT {IV}, SUM({CASE}) AS bp, COUNT({CASE}) AS n FROM a LEFT JOIN b ON {ON} GROUP BY {IV}",
    "weighted": f"SELECT a.name, SUM(b.score * ({OV})) AS w, AVG(b.score) AS m FROM a JOIN b ON {ON} GROUP BY a.name",
    "max_abs_difference": f"SELECT a.name, MAX(ABS(a.score - b.score)) AS d FROM a JOIN b ON {ON} GROUP BY a.name",
    "division": f"SELECT a.name, MIN(b.score / b.weight) AS r FROM a LEFT JOIN b ON {ON} GROUP BY a.name",
    "left_only_tree": f"SELECT a.name, SUM(a.end - a.start) AS len_ FROM a JOIN b ON {ON} GROUP BY a.name",
    "right_only_tree": f"SELECT a.name, SUM(b.end - b.start) AS len_ FROM a JOIN b ON {ON} GROUP BY a.name",
    "parenthesised_column": f"SELECT a.name, SUM((b.score)) AS s FROM a JOIN b ON {ON} GROUP BY a.name",
    "unary_minus": f"SELECT a.name, MIN(-b.score) AS s FROM a JOIN b ON {ON} GROUP BY a.name",
    "tail_on_the_alias": f"SELECT a.name, SUM({OV}) AS bp FROM a JOIN b ON {ON} AND a.strand = b.strand GROUP BY a.name "
                         "HAVING bp > 100 ORDER BY bp DESC LIMIT 3",
    "same_tree_twice": f"SELECT a.name, SUM({OV}) AS s, MAX({OV}) AS m, SUM(b.end - a.start) AS r FROM a JOIN b ON {ON} "
                       "GROUP BY a.name",
    "contains": f"SELECT {IV}, SUM(b.end - b.start) AS inner_bp FROM a JOIN b ON a.interval CONTAINS b.interval GROUP BY {IV}",
}

#: name -> (query, the start of its decline text with both opt-ins)
DECLINES = {
    "distinct": (f"SELECT a.name, SUM(DISTINCT {OV}) AS s FROM a JOIN b ON {ON} GROUP BY a.name", "SUM(DISTINCT <expression>)"),
    "constant": (f"SELECT a.name, SUM(1) AS s FROM a JOIN b ON {ON} GROUP BY a.name", "aggregate over a constant"),
    "constant_expression": (f"SELECT a.name, SUM(2 * 3) AS s FROM a JOIN b ON {ON} GROUP BY a.name",
                            "aggregate over a constant expression"),
    "string_valued": (f"SELECT a.name, MAX(LEAST(a.start, 'x')) AS s FROM a JOIN b ON {ON} GROUP BY a.name",
                      "aggregate over a string-valued expression"),
    "comparison": (f"SELECT a.name, SUM(a.start > b.start) AS s FROM a JOIN b ON {ON} GROUP BY a.name",
                   "comparison or boolean as the value of an aggregate"),
    "boolean": (f"SELECT a.name, SUM(NOT a.start) AS s FROM a JOIN b ON {ON} GROUP BY a.name",
                "comparison or boolean as the value of an aggregate"),
    "distance_argument": (f"SELECT a.name, SUM(DISTANCE(a.interval, b.interval)) AS s FROM a JOIN b ON {ON} GROUP BY a.name",
                          "DISTANCE inside an aggregate"),
    "distance_inside": (f"SELECT a.name, SUM(ABS(DISTANCE(a.interval, b.interval))) AS s FROM a JOIN b ON {ON} GROUP BY a.name",
                        "DISTANCE inside an aggregate over an expression"),
    "in_having": (f"SELECT a.name, COUNT(*) AS n FROM a JOIN b ON {ON} GROUP BY a.name HAVING SUM({OV}) > 3",
                  "aggregate over an expression in HAVING"),
    "in_order_by": (f"SELECT a.name, COUNT(*) AS n FROM a JOIN b ON {ON} GROUP BY a.name ORDER BY SUM({OV})",
                    "aggregate over an expression in ORDER BY"),
    "right_side_key": (f"SELECT b.name, SUM({OV}) AS s FROM a JOIN b ON {ON} GROUP BY b.name",
                       "aggregate over an expression outside the map shape"),
    "no_group_by": (f"SELECT SUM({OV}) AS s FROM a JOIN b ON {ON}", "aggregate over an expression outside the map shape"),
    "unaliased": (f"SELECT a.name, SUM({OV}) FROM a JOIN b ON {ON} GROUP BY a.name",
                  "aggregate over an expression outside the map shape"),
    "left_with_where": (f"SELECT a.name, SUM({OV}) AS s FROM a LEFT JOIN b ON {ON} WHERE a.score > 3 GROUP BY a.name",
                        "aggregate over an expression outside the map shape"),
    "semi_join": (f"SELECT a.name, SUM(a.end - a.start) AS s FROM a SEMI JOIN b ON {ON} GROUP BY a.name",
                  "aggregate over an expression outside the map shape"),
    "nine_aggregates": ("SELECT a.name, " + ", ".join(f"SUM(b.score + {i}) AS s{i}" for i in range(9))
                        + f" FROM a JOIN b ON {ON} GROUP BY a.name", "aggregate over an expression outside the map shape"),
    "modulo": (f"SELECT a.name, SUM(b.start % 2) AS s FROM a JOIN b ON {ON} GROUP BY a.name",
               "operator '%' in an expression inside an aggregate"),
    "function_call": (f"SELECT a.name, SUM(SQRT(b.score)) AS s FROM a JOIN b ON {ON} GROUP BY a.name",
                      "function call in an expression inside an aggregate"),
}

#: name -> query without an aggregate over an expression: both opt-ins change nothing beyond ``join_aggregates`` alone
NEIGHBOURS = {
    "column_aggregates": f"SELECT {IV}, AVG(b.score) AS mean, COUNT(b.score) AS n FROM a LEFT JOIN b ON {ON} GROUP BY {IV}",
    "computed_column": f"SELECT a.name, {OV} AS overlap_bp FROM a JOIN b ON {ON}",
    "computed_column_beside_aggregate": f"SELECT a.name, {OV} AS overlap_bp, SUM(b.score) AS s FROM a JOIN b ON {ON} GROUP BY a.name",
    "count_star_argument": f"SELECT a.name, SUM(*) AS s FROM a JOIN b ON {ON} GROUP BY a.name",
    "star_argument": f"SELECT a.name, COUNT(b.*) AS s FROM a JOIN b ON {ON} GROUP BY a.name",
    "window": f"SELECT a.name, SUM(b.score) OVER () AS s FROM a JOIN b ON {ON}",
    "order_by_plain_aggregate": f"SELECT a.name, COUNT(*) AS n FROM a JOIN b ON {ON} GROUP BY a.name ORDER BY SUM(b.score)",
}

ALL = {**IN_SHAPE, **{k: v[0] for k, v in DECLINES.items()}, **NEIGHBOURS}

#: the opt-ins of the commit before ``aggregate_expressions`` that every query was recorded under
OPTIONS = {
    "plain": {},
    "join_aggregates": {"join_aggregates": True},
    "select_expressions": {"select_expressions": True},
    "both_older": {"join_aggregates": True, "select_expressions": True},
    "outer_joins": {"outer_joins": True},
}


def outcome(build_plan, query: str, **opts) -> dict:
    """What ``build_plan`` makes of a query: ``{"plan": <string form>}`` or ``{"error": <class name>, "message": ...}``."""
    try:
        return {"plan": build_plan(query, TABLES, **opts).to_string()}
    except ValueError as exc:       # (HipDeclined is one)
        return {"error": type(exc).__name__, "message": str(exc)}
