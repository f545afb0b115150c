"""The ``dialect="hip"`` lowering target: a serialisable join plan.

Where the reference's DuckDB override emits a verbatim SQL payload through
``exp.Command`` (``src/giql/expanders/intersects_duckdb.py:1713``), the hip target
emits this plan's string form; :func:`giql_amd.execute.execute` turns plan +
Arrow tables into one C-ABI call.  sqlglot-free.
"""

from __future__ import annotations

import json
from dataclasses import asdict, dataclass, field

PLAN_PREFIX = "GIQL-HIP-PLAN/1 "

KINDS = ("INNER", "SEMI", "ANTI", "NEAREST", "COUNT", "CLUSTER", "MERGE", "FILTER", "DISJOIN", "LEFT")

#: the kinds that produce pairs through a spatial predicate: INNER, and LEFT = INNER's pairs + one (left row, NULL)
#: row per left row that keeps none (its ON residuals take part in matching, its WHERE residuals filter the result)
PAIR_KINDS = ("INNER", "LEFT")

#: the kinds that keep one flag or one integer per left row
ROW_KINDS = ("SEMI", "ANTI", "COUNT")

#: the spatial predicate of an INNER plan
PREDICATES = ("intersects", "contains", "within", "within_distance")

#: the three columns DISJOIN appends to the target's row (src/giql/expanders/disjoin.py:191-198)
DISJOIN_COLUMNS = ("disjoin_chrom", "disjoin_start", "disjoin_end")

#: what JoinPlan.segments may say: the query forms answered from a table's coverage segments
SEGMENT_FORMS = ("distinct", "depth", "runs")


@dataclass(frozen=True)
class PlanSide:
    """One operand: the table's physical columns and its coordinate encoding
    (what ``_build_sql`` reads from ``self.tables``, intersects_duckdb.py:1179-1188)."""

    table: str
    alias: str
    chrom_col: str = "chrom"
    start_col: str = "start"
    end_col: str = "end"
    coordinate_system: str = "0based"
    interval_type: str = "half_open"

    @property
    def encoding(self) -> tuple[str, str]:
        return (self.coordinate_system, self.interval_type)


@dataclass(frozen=True)
class Projection:
    side: str      # "l", "r", "distance" (NEAREST), "count" (COUNT aggregate); "pair_distance" (INNER: the
                   # DISTANCE of the pair as a nullable int64 column; column = "lr" | "rl" -- which table is the
                   # CASE's A operand -- then "+signed" / "+stranded", src/giql/expanders/_distance.py:67-117);
                   # "expr" (INNER / LEFT: a computed column, column = the index into JoinPlan.expressions as text);
                   # "l" / "r" with column "*" (beside a computed column only): every column of that table, by name;
                   # CLUSTER / MERGE:
                   # "star" (every table column), "cluster" (the id), "count" (COUNT(*)), "agg" (MERGE: an
                   # aggregate of a value column, column = the index into JoinPlan.aggregates as text); DISJOIN: "l" (a
                   # target column), "disjoin" (column = one of DISJOIN_COLUMNS), "star" (the target's
                   # columns, then the three); a plan with ``segments`` set: "disjoin" and "count" (COUNT(*)) only
    column: str
    name: str      # output column name


@dataclass(frozen=True)
class Operand:
    """One side of a residual comparison: a column of the left / right table
    (``kind`` "l" / "r", ``value`` = column name) or a literal ("int", "float", "str")."""

    kind: str
    value: object


@dataclass(frozen=True)
class Residual:
    """An extra conjunct beside the INTERSECTS: ``lhs op rhs`` from the ON or the
    WHERE clause (the reference inlines these into the per-chromosome join,
    intersects_duckdb.py:1157-1177, 1239-1243)."""

    clause: str    # "on" | "where"
    lhs: Operand
    op: str        # = != < <= > >= isnull notnull (the last two read lhs only)
    rhs: Operand
    group: int = 0  # residuals are AND-ed; those sharing a non-zero group are OR-ed (one CNF clause)


@dataclass(frozen=True)
class Aggregate:
    """A plain aggregate of the outer SELECT (``FUNC([DISTINCT] <col>)`` or ``COUNT(*)``), computed
    over the join's rows per ``group_by`` key (the reference rebuilds these over its wrapper
    relation, intersects_duckdb.py:1402-1644)."""

    func: str      # COUNT SUM MIN MAX AVG; beside MERGE also STRING_AGG
    side: str      # "l" / "r", or "*" for COUNT(*); "x": an expression over the pair, ``column`` its index into
                   # JoinPlan.expressions as text (a map-shape plan lowered with the ``aggregate_expressions`` opt-in)
    column: str
    name: str      # output column name
    distinct: bool = False
    # STRING_AGG beside MERGE only (a plan lowered with the ``string_aggregates`` opt-in): the literal separator.
    # None for every other aggregate; plan strings written before the field existed load with None
    separator: str | None = None


@dataclass(frozen=True)
class Having:
    """One conjunct of the HAVING clause over the grouped result: ``lhs op rhs`` where an operand is an
    output column of the grouping (``kind`` "name": a key, an aggregate of the SELECT list, or a hidden
    ``__giql_h<n>`` aggregate computed for this clause only) or a literal ("int", "float", "str")."""

    lhs: Operand
    op: str        # = != < <= > >= isnull notnull
    rhs: Operand
    group: int = 0  # conjuncts sharing a non-zero group are OR-ed (one clause of the normal form)


#: the operators and quantifiers of a literal range set
RANGE_OPS = ("intersects", "contains", "within")
RANGE_QUANTIFIERS = ("any", "all")


@dataclass(frozen=True)
class RangeSet:
    """``<genomic column> <op> ANY | ALL ('chr:lo-hi', ...)`` over a FILTER plan's table, or its negation
    (docs/dialect/quantifiers.rst; src/giql/expanders/intersects.py:243-270): one term ``chrom = c AND <cmp on start>
    AND <cmp on end>`` per range, OR-ed for ANY and AND-ed for ALL, in three-valued logic.  SOME is ANY."""

    op: str                    # intersects | contains | within
    quantifier: str            # any | all
    negated: bool
    ranges: tuple              # (chrom, start, end) per range, canonical 0-based half-open


@dataclass(frozen=True)
class JoinPlan:
    kind: str
    left: PlanSide
    right: PlanSide | None      # None for the single-table operators (CLUSTER / MERGE / FILTER) and for
                                # DISJOIN in self mode (the reference defaults to the target)
    projection: tuple[Projection, ...] = field(default_factory=tuple)
    distinct: bool = False
    # NEAREST only (src/giql/expanders/nearest.py:240-252)
    k: int = 1
    max_distance: int | None = None
    signed: bool = False
    residuals: tuple[Residual, ...] = field(default_factory=tuple)
    # CLUSTER / MERGE only (src/giql/expanders/cluster.py:222-243)
    distance: int = 0
    stranded: bool = False
    strand_col: str | None = None
    # CLUSTER(..., predicate := <comparison> [AND ...]) (src/giql/expanders/cluster.py:281-296): operand kind "l" = the
    # current row's column, "r" = PREV(column) -- the sorted predecessor's -- or a literal; clause "predicate"
    cluster_predicate: tuple[Residual, ...] = field(default_factory=tuple)
    # the clauses that ride on the reference's outer SELECT wrapper (intersects_duckdb.py:1336-1400),
    # finished on the projected table: projection columns named "__giql_*" are carried for them only
    # (a MERGE plan lowered with the ``merge_aggregates`` opt-in: the aggregates of value columns per merged region,
    # side "l", computed by HipEngine.merge_agg; a Projection("agg", "<index>", name) places each in the SELECT list)
    aggregates: tuple[Aggregate, ...] = field(default_factory=tuple)
    group_by: tuple[str, ...] = field(default_factory=tuple)       # output names of the key columns
    having: tuple[Having, ...] = field(default_factory=tuple)      # conjuncts over the grouped result
    # (output name, descending, NULLs first): the placement is explicit per key -- where the query does not
    # write NULLS FIRST / LAST it is giql's dialect default, "NULLs are small" (first when ascending, last
    # when descending), which the reference's emitted DuckDB SQL spells out the same way
    order_by: tuple[tuple[str, bool, bool], ...] = field(default_factory=tuple)
    limit: int | None = None
    offset: int | None = None
    output: tuple[str, ...] = field(default_factory=tuple)         # final column names in SELECT order (grouped plans)
    # INNER / LEFT only: the join's spatial predicate, left <predicate> right (src/giql/expanders/intersects.py:149-166).
    # "contains" / "within" run HipEngine.contain_join; plan strings written before the field existed load as
    # "intersects".  "within_distance": DISTANCE(left, right) <= max_distance (HipEngine.window_join; -1 = nothing
    # qualifies, the query compared with < 0).  A stranded "pair_distance" projection reads strand_col
    # ("<left column>,<right column>", as stranded NEAREST does)
    predicate: str = "intersects"
    # SEMI / ANTI / COUNT over "contains" / "within" / "within_distance" (HipEngine.semi_anti_pred / count_pred):
    # only plans lowered with the ``row_predicates`` opt-in carry such a predicate, and they say so here
    row_predicates: bool = False
    # INNER / LEFT only: the computed columns of the SELECT list (bedtools -wo / -wao: "LEAST(a.end, b.end) -
    # GREATEST(a.start, b.start) AS overlap_bp"), each an Operand("expr", tree) in the serialised form the residuals
    # use -- a searched CASE is ["fn", "if", [cond, then, else]], a missing ELSE ["fn", "null", []] -- evaluated per
    # result row by HipEngine.eval_exprs; a Projection("expr", "<index>", name) refers to one.  Only plans lowered with
    # the ``select_expressions`` opt-in carry any; plan strings written before the field existed load with none.
    # A map-shape plan (``join_aggregates``) lowered with the ``aggregate_expressions`` opt-in keeps here the trees its
    # aggregates of side "x" reduce (SUM(LEAST(a.end, b.end) - GREATEST(a.start, b.start))): no projection names them
    expressions: tuple[Operand, ...] = field(default_factory=tuple)
    # FILTER only: the literal range sets that HipEngine.range_set_any answers -- ANY over two or more ranges, or its
    # negation -- each one more conjunct beside the residuals (a single literal, ANY over one range, ALL and their
    # negations are folded into the residuals when the plan is lowered).  Only plans lowered with the ``range_sets``
    # opt-in carry any; plan strings written before the field existed load with none
    range_sets: tuple[RangeSet, ...] = field(default_factory=tuple)
    # INNER / LEFT only: a grouped plan in the map shape (shape.is_map_shape; bedtools ``map``) lowered with the
    # ``join_aggregates`` opt-in -- grouped by left-side columns, its aggregates over the right side computed per left
    # row on the device (HipEngine.pair_aggregate) and combined per key.  A LEFT plan so marked needs no padded pair.
    # The string form carries the key only when it is set: every other plan serialises as it did before the field
    join_aggregates: bool = False
    # DISJOIN in self mode only, lowered with the ``disjoin_aggregates`` opt-in: the query is answered from the coverage
    # segments of the target (HipEngine.coverage) instead of DISJOIN's per-piece rows.  "distinct": SELECT DISTINCT over
    # exactly the three disjoin_* columns; "depth": GROUP BY the three with COUNT(*) (a Projection("count", "*", name)
    # per count); "runs": MERGE(interval, predicate := depth = PREV(depth)) over the "depth" query as a sub-query --
    # abutting segments of equal depth merged, output chrom / start / end.  Absent from the string form when None
    segments: str | None = None

    def __post_init__(self) -> None:
        if self.kind not in KINDS:
            raise ValueError(f"unknown plan kind {self.kind!r}")
        if self.predicate not in PREDICATES:
            raise ValueError(f"unknown join predicate {self.predicate!r}")
        if self.row_predicates and (self.kind not in ROW_KINDS or self.predicate == "intersects"):
            raise ValueError("row_predicates marks a SEMI / ANTI / COUNT plan over CONTAINS / WITHIN / DISTANCE only")
        if self.predicate != "intersects" and self.kind not in PAIR_KINDS and not self.row_predicates:
            raise ValueError(f"predicate {self.predicate!r} needs an INNER plan, not {self.kind}")
        if self.predicate == "within_distance" and not isinstance(self.max_distance, int):
            raise ValueError("predicate 'within_distance' needs an integer max_distance")
        if self.expressions and self.kind not in PAIR_KINDS:
            raise ValueError(f"computed columns need an INNER or LEFT plan, not {self.kind}")
        if self.range_sets and self.kind != "FILTER":
            raise ValueError(f"literal range sets need a FILTER plan, not {self.kind}")
        if self.join_aggregates and not (self.kind in PAIR_KINDS and self.aggregates and self.group_by):
            raise ValueError("join_aggregates marks a grouped INNER / LEFT plan with aggregates only")
        if self.segments is not None and not (self.segments in SEGMENT_FORMS and self.kind == "DISJOIN"
                                              and self.right is None):
            raise ValueError(f"segments {self.segments!r} marks a self-mode DISJOIN plan as one of {SEGMENT_FORMS}")
        for rs in self.range_sets:
            if rs.op not in RANGE_OPS or rs.quantifier not in RANGE_QUANTIFIERS or not rs.ranges:
                raise ValueError(f"bad range set {rs.op!r} {rs.quantifier!r} over {len(rs.ranges)} ranges")
        for a in self.aggregates:
            if a.side == "x" and not (self.join_aggregates and a.column.isdigit() and int(a.column) < len(self.expressions)):
                raise ValueError(f"aggregate {a.name!r} names expression {a.column!r} of {len(self.expressions)} "
                                 "(a map-shape plan's aggregate over an expression)")
            if (a.func == "STRING_AGG") != (a.separator is not None) or (a.func == "STRING_AGG" and self.kind != "MERGE"):
                raise ValueError(f"aggregate {a.name!r}: STRING_AGG, and only STRING_AGG beside MERGE, carries a separator")
        for p in self.projection:
            if p.side == "agg" and not (self.kind == "MERGE" and p.column.isdigit()
                                        and int(p.column) < len(self.aggregates)):
                raise ValueError(f"projection {p.name!r} names aggregate {p.column!r} of {len(self.aggregates)}")
            if p.side == "expr" and not (p.column.isdigit() and int(p.column) < len(self.expressions)):
                raise ValueError(f"projection {p.name!r} names expression {p.column!r} of {len(self.expressions)}")

    def to_dict(self) -> dict:
        """The plan as plain JSON-able data (what :meth:`to_string` serialises)."""
        d = asdict(self)
        d["projection"] = [asdict(p) for p in self.projection]
        d["residuals"] = [asdict(r) for r in self.residuals]
        d["cluster_predicate"] = [asdict(r) for r in self.cluster_predicate]
        d["aggregates"] = [asdict(a) for a in self.aggregates]
        d["having"] = [asdict(h) for h in self.having]
        d["order_by"] = [list(o) for o in self.order_by]
        d["expressions"] = [asdict(e) for e in self.expressions]
        d["range_sets"] = [{"op": r.op, "quantifier": r.quantifier, "negated": r.negated,
                            "ranges": [list(t) for t in r.ranges]} for r in self.range_sets]
        if not self.join_aggregates:
            del d["join_aggregates"]
        if self.segments is None:
            del d["segments"]
        return d

    def to_string(self) -> str:
        return PLAN_PREFIX + json.dumps(self.to_dict(), sort_keys=True, separators=(",", ":"))

    @classmethod
    def from_string(cls, text: str) -> "JoinPlan":
        if not isinstance(text, str) or not text.startswith(PLAN_PREFIX):
            raise ValueError("not a GIQL hip plan string")
        return cls.from_dict(json.loads(text[len(PLAN_PREFIX):]))

    @classmethod
    def from_dict(cls, d: dict) -> "JoinPlan":
        return cls(
            kind=d["kind"], left=PlanSide(**d["left"]),
            right=PlanSide(**d["right"]) if d.get("right") else None,
            projection=tuple(Projection(**p) for p in d["projection"]),
            distinct=d.get("distinct", False), k=d.get("k", 1),
            max_distance=d.get("max_distance"), signed=d.get("signed", False),
            residuals=tuple(Residual(r["clause"], Operand(**r["lhs"]), r["op"], Operand(**r["rhs"]), r.get("group", 0))
                            for r in d.get("residuals", ())),
            distance=d.get("distance", 0), stranded=d.get("stranded", False), strand_col=d.get("strand_col"),
            cluster_predicate=tuple(Residual(r["clause"], Operand(**r["lhs"]), r["op"], Operand(**r["rhs"]), r.get("group", 0))
                                    for r in d.get("cluster_predicate", ())),
            aggregates=tuple(Aggregate(**a) for a in d.get("aggregates", ())),
            having=tuple(Having(Operand(**h["lhs"]), h["op"], Operand(**h["rhs"]), h.get("group", 0))
                         for h in d.get("having", ())),
            group_by=tuple(d.get("group_by", ())),
            order_by=tuple((o[0], bool(o[1]), bool(o[2]) if len(o) > 2 else not bool(o[1])) for o in d.get("order_by", ())),
            limit=d.get("limit"), offset=d.get("offset"), output=tuple(d.get("output", ())),
            predicate=d.get("predicate", "intersects"), row_predicates=d.get("row_predicates", False),
            expressions=tuple(Operand(**e) for e in d.get("expressions", ())),
            range_sets=tuple(RangeSet(r["op"], r["quantifier"], bool(r["negated"]),
                                      tuple((str(c), int(lo), int(hi)) for c, lo, hi in r["ranges"]))
                             for r in d.get("range_sets", ())),
            join_aggregates=bool(d.get("join_aggregates", False)), segments=d.get("segments"))


def is_plan_string(text) -> bool:
    return isinstance(text, str) and text.startswith(PLAN_PREFIX)
