"""The shape gate of ``dialect="hip"``: ONE function over a small neutral description of a
two-table INTERSECTS statement, shared by the two front ends that can produce it --

* :mod:`giql_amd.transpile` (the sqlglot-free mirror: tokens -> :class:`JoinShape`), and
* :mod:`giql_amd.plugin` (giql's own ``@register(HipTarget, Intersects)`` hook: sqlglot AST +
  ``ExpansionContext`` -> :class:`JoinShape`),

so both accept, decline and reject exactly the same queries.  It restates the whitelist of
``IntersectsDuckDBIEJoinTransformer.transform_to_sql`` / ``_build_sql``
(``src/giql/expanders/intersects_duckdb.py:618-804, 1136-1400``):

* one column-to-column INTERSECTS between two distinct registered-or-default base tables, joined
  INNER / CROSS / comma / SEMI / ANTI (or the count_overlaps ``LEFT JOIN ... COUNT(b.col) ...
  GROUP BY`` shape, ``:432-548``), optionally ``USING (<chrom>)`` (``:727-735, 1190-1201``);
* residual conditions beside it -- comparisons over columns, literals and arithmetic in conjunctive normal form
  (ON residuals join, WHERE residuals filter: ``:889-912, 1164-1177``);
* a projection of qualified columns and plain aggregates (``:1402-1644``); stars, expressions,
  windows, FILTER, sub-queries decline (#202, #204, #205);
* DISTINCT / GROUP BY / ORDER BY / LIMIT / OFFSET over the result, which the reference lets "ride on
  the outer SELECT wrapper" (``:1336-1400``) and this target finishes on the projected Arrow table
  (:func:`giql_amd.execute.execute`); HAVING as a conjunction of comparisons between aggregates / keys
  and literals; DISTINCT ON, sub-queries and expressions decline.

Errors follow the reference's convention: user mistakes (unqualified / unknown-qualifier columns,
right-side columns under SEMI / ANTI) are ``ValueError``; valid GIQL this target does not run is
:class:`HipDeclined` (the reference *declines* such shapes to the naive predicate, ``:1715``).
"""

from __future__ import annotations

from dataclasses import dataclass, field

from .plan import DISJOIN_COLUMNS, Aggregate, Having, JoinPlan, Operand, PlanSide, Projection, Residual
from .table import Table, Tables


class HipDeclined(ValueError):
    """Valid GIQL that the hip dialect does not execute (reference: decline)."""


def decline(reason: str) -> HipDeclined:
    return HipDeclined(
        f"{reason}: this query shape is valid GIQL but is not executed by dialect='hip' "
        "(the reference declines it to the naive overlap predicate); transpile it with "
        "giql.transpile(...) for a SQL engine instead")


# ------------------------------------------------------- boolean conditions -> CNF
# Both front ends hand a condition over as a tree -- ("leaf", term) | ("and", [nodes]) |
# ("or", [nodes]) | ("not", node), a term being a spatial predicate (SPATIAL_TERMS: ("intersects", ...),
# ("contains", ...), ("within", ...), their literal-range forms ("intersects_lit", ...) ..., or -- from a parser with
# the ``range_sets`` opt-in -- ("range_set", op, quantifier, ColRef, literals, negated))
# or ("cmp", lhs, op, rhs) -- and get the terms of its conjunctive normal form back: the
# select kernel evaluates an AND of ORs (include/giql_hip.h, giql_pred.group).  The
# reference inlines such extras as SQL text (_classify_extras, intersects_duckdb.py:889-912).
#: the column-to-column spatial predicates a join may carry (src/giql/expanders/intersects.py:149-166): a term
#: (name, ColRef, ColRef) read "lhs <name> rhs"
SPATIAL_TERMS = ("intersects", "contains", "within")
#: DISTANCE(x.interval, y.interval) <= N as a join predicate (docs/recipes/distance.rst:60-73): a term
#: ("within_distance", ColRef, ColRef, N) with N already the inclusive bound (-1: nothing qualifies)
DISTANCE_TERM = "within_distance"
JOIN_TERMS = SPATIAL_TERMS + (DISTANCE_TERM,)
_FLIPPED = {"intersects": "intersects", "contains": "within", "within": "contains", DISTANCE_TERM: DISTANCE_TERM}
NEGATED_OP = {"=": "!=", "!=": "=", "<": ">=", ">=": "<", ">": "<=", "<=": ">", "isnull": "notnull",
              "notnull": "isnull"}
MAX_CONDITION_LEAVES = 12   # a select call takes 16 predicates; a literal-range filter adds three of its own


_MIRRORED_OP = {"<": ">", "<=": ">=", ">": "<", ">=": "<=", "=": "=", "!=": "!="}
INT64_MAX = (1 << 63) - 1


def holds_distance(o) -> bool:
    """Does an operand term hold a DISTANCE call -- ``("distfn", ColRef, ColRef, stranded, signed)`` -- anywhere?"""
    if o[0] == "distfn":
        return True
    return o[0] == "fn" and any(holds_distance(c) for c in o[2])


def comparison_leaf(lhs, op, rhs):
    """The condition-tree leaf of ``lhs op rhs``.  Both front ends build every comparison through here, so a
    DISTANCE call among the operands is met in ONE place: ``DISTANCE(x.interval, y.interval) <= N`` / ``< N``
    (N an integer literal; also written ``N >= DISTANCE(...)``) becomes the join predicate
    ``("within_distance", x, y, bound)``; every other use of the value in a condition declines -- the reference
    evaluates its CASE row by row over a cartesian product there (docs/dialect/distance-operators.rst:68-78)."""
    if not (holds_distance(lhs) or holds_distance(rhs)):
        return ("leaf", ("cmp", lhs, op, rhs))
    if lhs[0] != "distfn" and rhs[0] == "distfn":
        lhs, rhs, op = rhs, lhs, _MIRRORED_OP.get(op, op)
    if lhs[0] != "distfn":
        raise decline("DISTANCE inside an arithmetic expression of a condition")
    if op in ("isnull", "notnull"):
        raise decline("IS [NOT] NULL over a DISTANCE")
    if op not in ("<", "<="):
        raise decline(f"DISTANCE compared with {op} (only DISTANCE(...) <= N and < N run as a join)")
    if rhs[0] != "lit" or isinstance(rhs[1], bool) or not isinstance(rhs[1], int):
        raise decline("DISTANCE bound that is not an integer literal")
    _, a, b, stranded, signed = lhs
    if stranded or signed:
        raise decline("signed / stranded DISTANCE in a join condition")
    bound = rhs[1] - (1 if op == "<" else 0)
    if bound > INT64_MAX:
        raise decline("DISTANCE bound that does not fit int64")
    return ("leaf", (DISTANCE_TERM, a, b, max(bound, -1)))


def _nnf(node, neg: bool = False):
    """Push NOT down to the comparisons.  Exact under three-valued logic: a filter keeps TRUE
    only, De Morgan holds in Kleene logic and NOT (x < y) is TRUE exactly when x >= y is."""
    k = node[0]
    if k == "leaf":
        if not neg:
            return node
        t = node[1]
        if t[0] == "range_set":     # (only a parser with the ``range_sets`` opt-in builds this term: its last field flips)
            return ("leaf", t[:-1] + (not t[-1],))
        if t[0] != "cmp":
            raise decline("NOT over a spatial predicate")
        return ("leaf", ("cmp", t[1], NEGATED_OP[t[2]], t[3]))
    if k == "not":
        return _nnf(node[1], not neg)
    kids = [_nnf(c, neg) for c in node[1]]
    return (("or" if k == "and" else "and") if neg else k, kids)


def _cnf(node) -> list:
    k = node[0]
    if k == "leaf":
        return [[node[1]]]
    if k == "and":
        return [cl for c in node[1] for cl in _cnf(c)]
    acc = [[]]
    for c in node[1]:
        acc = [a + cl for a in acc for cl in _cnf(c)]
        if sum(len(a) for a in acc) > 4 * MAX_CONDITION_LEAVES:
            raise decline("condition too large once normalised")
    return acc


def _bool_term(node):
    """A (NOT-free) condition node as an operand term ``("fn", op, [args])`` for the select kernel's boolean
    programs: comparisons, IS [NOT] NULL, AND / OR (``giql_hip_select_expr_dev``, GIQL_X_EQ .. GIQL_X_OR)."""
    k = node[0]
    if k == "leaf":
        t = node[1]
        if t[0] != "cmp":
            raise decline("spatial predicate under OR")
        if t[2] in ("isnull", "notnull"):
            return ("fn", t[2], [t[1]])
        return ("fn", t[2], [t[1], t[3]])
    return ("fn", k, [_bool_term(c) for c in node[1]])


def condition_terms(tree, trees: bool = False) -> list:
    """The condition's CNF as terms: a one-leaf clause is the leaf itself, a longer one
    ``("or", [cmp, ...])``.  A spatial predicate must be a conjunct of its own (under OR / NOT
    the reference falls back too: ``_classify_extras``).

    ``trees`` (the join's residuals, round 4): a condition whose normal form outgrows the cap is not declined --
    its top-level conjuncts stay as they are, a plain comparison a term as before, anything nested ONE term
    ``("tree", ("fn", op, [...]))`` that the select kernel evaluates as a boolean program under three-valued
    logic (the reference inlines such a condition as text, intersects_duckdb.py:889-957).  Small conditions keep
    their normal form: its clauses are what places a one-table condition BEFORE the join."""
    nnf = _nnf(tree)
    if trees:
        try:
            return condition_terms(tree)
        except HipDeclined as exc:
            if "too large" not in str(exc):
                raise
        out = []
        stack = [nnf]
        conjuncts = []
        while stack:                      # the top-level ANDs, in order
            n = stack.pop()
            if n[0] == "and":
                stack.extend(reversed(n[1]))
            else:
                conjuncts.append(n)
        for n in conjuncts:
            out.append(n[1] if n[0] == "leaf" else ("tree", _bool_term(n)))
        return out
    out, leaves = [], 0
    for clause in _cnf(nnf):
        uniq = []
        for t in clause:
            if t not in uniq:
                uniq.append(t)
        if len(uniq) == 1:
            out.append(uniq[0])
        else:
            if any(t[0] != "cmp" for t in uniq):
                raise decline("spatial predicate under OR")
            out.append(("or", uniq))
        leaves += sum(t[0] == "cmp" for t in uniq)
    if leaves > MAX_CONDITION_LEAVES:
        raise decline("condition too large once normalised")
    return out


def norm(name: str, quoted: bool = False) -> str:
    # unquoted identifiers are case-insensitive (intersects_duckdb.py:119-128)
    return name if quoted else name.casefold()


AGG_FUNCS = ("COUNT", "SUM", "MIN", "MAX", "AVG")


# ------------------------------------------------------------- the description
@dataclass
class ColRef:
    table: str | None
    table_quoted: bool
    column: str
    star: bool = False
    count: bool = False  # COUNT(<this column>) -- kept for the count_overlaps shape


@dataclass
class TableRef:
    name: str
    alias: str
    alias_quoted: bool = False


@dataclass
class SelItem:
    """One SELECT-list item: a column, or a plain aggregate ``FUNC([DISTINCT] <col> | *)``."""

    ref: ColRef | None           # the column / the aggregate's argument (None: COUNT(*))
    alias: str | None = None
    func: str | None = None      # None = plain column
    distinct: bool = False
    # DISTANCE(x.interval, y.interval [, stranded := b] [, signed := b]) as an output column: (ColRef x, ColRef y,
    # stranded, signed); ``ref`` is None then
    distance: tuple | None = None
    # a computed column (``select_expressions``): an operand term as the residuals' operands are -- ("col", ColRef) /
    # ("lit", v) / ("fn", op, [terms]), a searched CASE as ("fn", "if", [condition, then, else]) over a condition
    # term (``case_term``), a missing ELSE as ("fn", "null", []); ``ref`` is None then and ``alias`` is set.  With
    # ``func`` set too (``aggregate_expressions``): the argument of that aggregate, ``SUM(<expr>)``
    expr: tuple | None = None


@dataclass
class OrderKey:
    ref: ColRef                  # qualified column, or an output name (table None)
    desc: bool = False
    nulls_first: bool | None = None   # NULLS FIRST / NULLS LAST; None = not written (giql's dialect default: NULLs are small)


@dataclass
class JoinShape:
    """What either front end hands to :func:`lower_join_shape`."""

    items: list[SelItem]
    from_ref: TableRef
    join_ref: TableRef
    kind: str = "INNER"                      # INNER (also CROSS / comma) | SEMI | ANTI | LEFT
    on_seen: bool = False
    # ("intersects", ColRef, ColRef) | ("cmp", lhs, op, rhs) | ("or", [cmp, ...]) | ("tree", boolean program): see condition_terms
    on_terms: list = field(default_factory=list)
    where_terms: list = field(default_factory=list)
    using: list[str] = field(default_factory=list)
    distinct: bool = False
    group_by: list[ColRef] = field(default_factory=list)
    # HAVING terms ("cmp", lhs, op, rhs) | ("or", [cmp, ...]); an operand is ("lit", value), ("col", ColRef) or ("agg", SelItem)
    having: list = field(default_factory=list)
    order_by: list[OrderKey] = field(default_factory=list)
    limit: int | None = None
    offset: int | None = None
    # the two operands as resolved by the caller (the plugin reads them from
    # ``ctx.resolution.column(...)``); None = derive them from ``tables`` by table name
    sides: tuple[PlanSide, PlanSide] | None = None
    # opt-in: a LEFT [OUTER] JOIN outside the count_overlaps shape lowers to a LEFT plan instead of declining
    outer_joins: bool = False
    # opt-in: SEMI / ANTI joins and the count_overlaps shape over CONTAINS / WITHIN / DISTANCE <= N lower to SEMI /
    # ANTI / COUNT plans carrying that predicate instead of declining
    row_predicates: bool = False
    # opt-in: arithmetic / searched-CASE items of the SELECT list (SelItem.expr) lower to computed columns of an INNER
    # or LEFT plan; a front end that does not parse them never sets SelItem.expr
    select_expressions: bool = False
    # opt-in: a grouped aggregate over a join in the map shape (is_map_shape) lowers to an INNER / LEFT plan marked
    # ``join_aggregates``, whose aggregates execute() computes per left row on the device (HipEngine.pair_aggregate)
    join_aggregates: bool = False
    # opt-in, together with ``join_aggregates``: an aggregate of the map shape may take an expression over both tables
    # (SelItem.func AND SelItem.expr set); a front end that does not parse them never sets both
    aggregate_expressions: bool = False


# ------------------------------------------------------------------ helpers
def table_side(ref: TableRef, tables: Tables) -> PlanSide:
    t = tables.get(ref.name)
    if t is None:
        # an unregistered table uses default column names, like the naive plan
        # (intersects_duckdb.py:1179-1188)
        t = Table(ref.name)
    return PlanSide(table=ref.name, alias=norm(ref.alias, ref.alias_quoted),
                    chrom_col=t.chrom_col, start_col=t.start_col, end_col=t.end_col,
                    coordinate_system=t.coordinate_system, interval_type=t.interval_type)


def genomic_col(name: str, tables: Tables) -> str:
    t = tables.get(name)
    return t.genomic_col if t is not None else "interval"


def _side_of(ref: ColRef, left: PlanSide, right: PlanSide, where: str) -> str:
    if ref.table is None:
        raise ValueError(
            f"Unqualified column {ref.column!r} in {where}: the hip join path has no live schema to "
            "attribute it to a side; it must be qualified with a table alias")
    q = norm(ref.table, ref.table_quoted)
    if q == left.alias:
        return "l"
    if q == right.alias:
        return "r"
    raise ValueError(f"Unknown table qualifier {ref.table!r} in {where}")


def distance_projection(it: SelItem, left: PlanSide, right: PlanSide, tables: Tables) -> tuple:
    """A DISTANCE select item -> ``(Projection("pair_distance", code, name), strand columns | None)``.  ``code``
    says which table is the CASE's A operand -- "lr": the left one, "rl": the right one (the sign and the strand
    flip follow A, src/giql/expanders/_distance.py:88-117) -- followed by "+signed" / "+stranded" as asked."""
    x, y, stranded, signed = it.distance
    for ref in (x, y):
        if ref.star or ref.table is None:
            raise decline("DISTANCE operand that is not a table-qualified column")
    sx, sy = _side_of(x, left, right, "DISTANCE"), _side_of(y, left, right, "DISTANCE")
    if sx == sy:
        raise decline("DISTANCE between two columns of one table")
    for ref, sd in ((x, sx), (y, sy)):
        table = left.table if sd == "l" else right.table
        if ref.column != genomic_col(table, tables):
            raise ValueError(f"DISTANCE operands must be the tables' genomic columns "
                             f"({genomic_col(left.table, tables)!r} / {genomic_col(right.table, tables)!r})")
    strands = None
    if stranded:
        cols = []
        for side in (left, right):
            t = tables.get(side.table)
            cols.append(t.strand_col if t is not None else "strand")
        if not all(cols):
            raise decline("stranded DISTANCE over a table without a strand column")
        strands = ",".join(cols)
    code = ("lr" if sx == "l" else "rl") + ("+signed" if signed else "") + ("+stranded" if stranded else "")
    return Projection("pair_distance", code, it.alias or "distance"), strands


def resolve_projection(items, left: PlanSide, right: PlanSide, left_only: bool,
                       distance_alias: str | None = None, tables: Tables | None = None,
                       strands_out: list | None = None, exprs_out: list | None = None,
                       stars: bool = False) -> tuple[Projection, ...]:
    """``strands_out`` (a list) receives the "<left>,<right>" strand columns of every stranded DISTANCE item,
    ``exprs_out`` the bound expression of every computed column, in the order their projections number them.
    ``stars``: a qualified star lowers to ``Projection(side, "*", "*")`` instead of declining."""
    out = []
    for it in items:
        ref = it.ref
        if it.distance is not None:
            if tables is None:      # (NEAREST: its own ``distance`` column is the one it offers)
                raise decline("DISTANCE in the SELECT list of a NEAREST join")
            proj, strands = distance_projection(it, left, right, tables)
            out.append(proj)
            if strands and strands_out is not None:
                strands_out.append(strands)
            continue
        if it.expr is not None:
            if exprs_out is None:
                raise decline("expression in the SELECT list of a NEAREST join")
            out.append(Projection("expr", str(len(exprs_out)), it.alias))
            exprs_out.append(expression_operand(it, left, right))
            continue
        if it.func is not None or ref.count:
            raise decline("COUNT(...) outside the count_overlaps LEFT JOIN ... GROUP BY shape")
        if ref.star and stars and ref.table is not None and not it.alias:
            # a.* / b.* beside a computed column (the -wo / -wao recipes, ``select_expressions``): execute() has the
            # table and enumerates its columns there, so nothing is narrowed
            out.append(Projection(_side_of(ref, left, right, "the SELECT list"), "*", "*"))
            continue
        if ref.star:
            # schema-less star enumeration would narrow the result (#202)
            raise decline("star projection")
        side = _side_of(ref, left, right, "the SELECT list")
        name = it.alias or ref.column
        if side == "l":
            out.append(Projection("l", ref.column, name))
        elif left_only:
            raise ValueError(
                f"Column {ref.table}.{ref.column} references the right side of a SEMI/ANTI "
                "join, which is out of scope in the SELECT list (left-side columns only)")
        elif distance_alias is not None and ref.column == "distance":
            out.append(Projection("distance", "distance", name))
        else:
            out.append(Projection("r", ref.column, name))
    return tuple(out)


COMPARISONS = ("=", "!=", "<", "<=", ">", ">=", "isnull", "notnull")


def bind_expression(o, bind_leaf) -> Operand:
    """An operand term -- ``("lit", v)`` / a column term / ``("fn", op, [terms])`` -- as a plan operand; columns and
    literals through ``bind_leaf``.  Arithmetic becomes ``Operand("expr", ["fn", op, [children]])`` whose leaves
    are ``[kind, value]`` pairs (lists throughout: the plan's JSON form gives lists back)."""
    if holds_distance(o):
        # (comparison_leaf turns the one accepted use into a join predicate before any operand is bound; whatever still
        # carries a call here came past it, and a "distfn" term must never be read as a column term)
        raise decline("DISTANCE as an operand of a condition (only DISTANCE(...) <= N and < N run, as a join)")
    if o[0] != "fn":
        return bind_leaf(o)

    def tree(t, strings_ok=False):
        if t[0] == "fn":
            cmp = t[1] in COMPARISONS       # (strings compare and can be NULL; they take no part in arithmetic)
            return ["fn", t[1], [tree(c, cmp) for c in t[2]]]
        leaf = bind_leaf(t)
        if leaf.kind == "str" and not strings_ok:
            raise ValueError(f"a string ({leaf.value!r}) cannot take part in arithmetic")
        return [leaf.kind, leaf.value]

    return Operand("expr", tree(o))


def operand_sides(o: Operand) -> set:
    """The tables ("l" / "r") an operand reads."""
    if o.kind in ("l", "r"):
        return {o.kind}
    if o.kind != "expr":
        return set()

    def walk(t):
        if t[0] == "fn":
            return set().union(*[walk(c) for c in t[2]]) if t[2] else set()
        return {t[0]} if t[0] in ("l", "r") else set()

    return walk(o.value)


#: what one call of the select kernel takes (``check_program`` in ``csrc/giql_hip.hip``: ``SEL_X_STACK`` values
#: live, 64 postfix nodes per call): the gate declines what the target cannot run instead of failing at run time
MAX_EXPR_DEPTH = 12
MAX_EXPR_NODES = 256


def expression_cost(o: Operand) -> tuple:
    """``(postfix nodes, values live at once)`` of an operand as ``HipEngine._flatten_expr`` lays it out: a leaf is
    one node and one value; an n-ary function folds pairwise (n - 1 operator nodes, its first argument's result
    stays on the stack while the next is evaluated); a unary one adds a node."""
    if o.kind != "expr":
        return (0, 0)

    def walk(t):
        if t[0] != "fn":
            return (1, 1)
        kids = [walk(c) for c in t[2]]
        if not kids:
            return (1, 1)
        if t[1] == "if":    # cond, then, else, IF: the condition and `then` stay live while `else` is evaluated
            return (sum(k[0] for k in kids) + 1, max(k[1] + i for i, k in enumerate(kids)))
        nodes = sum(k[0] for k in kids) + max(len(kids) - 1, 1)
        depth = max([kids[0][1]] + [1 + k[1] for k in kids[1:]])
        return (nodes, depth)

    return walk(o.value)


def case_term(whens, otherwise):
    """A searched CASE -- ``[(condition tree, value term), ...]`` and the ELSE term or None -- as the operand term
    ``("fn", "if", [condition, then, else])``, nested WHEN by WHEN; a missing ELSE is ``("fn", "null", [])``.  A
    condition is what ``condition_terms`` takes, except a spatial predicate: NOT is pushed into the comparisons
    (exact: ``if`` takes ``then`` only where the condition is TRUE, as a filter keeps only TRUE) and the rest becomes
    a boolean term of the select kernel's programs."""
    out = otherwise if otherwise is not None else ("fn", "null", [])
    for cond, value in reversed(whens):
        for leaf in _leaves(cond):
            if leaf[0] == DISTANCE_TERM:
                raise decline("DISTANCE inside an expression of the SELECT list")
            if leaf[0] != "cmp":
                raise decline("spatial predicate in a CASE condition")
        out = ("fn", "if", [_bool_term(_nnf(cond)), value, out])
    return out


def _leaves(node):
    if node[0] == "leaf":
        yield node[1]
    elif node[0] == "not":
        yield from _leaves(node[1])
    else:
        for c in node[1]:
            yield from _leaves(c)


def _string_valued(t, under_cmp: bool = False) -> bool:
    """Does a string literal stand anywhere but directly under a comparison?"""
    if t[0] == "lit":
        return isinstance(t[1], str) and not under_cmp
    if t[0] != "fn":
        return False
    return any(_string_valued(c, t[1] in COMPARISONS) for c in t[2])


def expression_operand(it: SelItem, left: PlanSide, right: PlanSide) -> Operand:
    """A computed column's term bound to the two sides: ``Operand("expr", tree)``, the form residual operands have."""
    if holds_distance(it.expr):
        raise decline("DISTANCE inside an expression of the SELECT list")
    if _string_valued(it.expr):
        raise decline("string-valued expression in the SELECT list")

    def bind(o) -> Operand:
        if o[0] == "lit":
            v = o[1]
            return Operand("str" if isinstance(v, str) else ("float" if isinstance(v, float) else "int"), v)
        ref: ColRef = o[1]
        if ref.star:
            raise decline("star in an expression of the SELECT list")
        return Operand(_side_of(ref, left, right, "the SELECT list"), ref.column)

    op = bind_expression(it.expr, bind)
    if not operand_sides(op):
        raise decline("constant expression in the SELECT list")
    nodes, depth = expression_cost(op)
    if depth > MAX_EXPR_DEPTH:
        raise decline(f"expression too deep for the eval kernel ({depth} values live, at most {MAX_EXPR_DEPTH})")
    if nodes > MAX_EXPR_NODES:
        raise decline(f"expression too large for one eval call ({nodes} nodes, at most {MAX_EXPR_NODES})")
    return op


def aggregate_operand(it: SelItem, left: PlanSide, right: PlanSide) -> Operand:
    """The argument of an aggregate over an expression (``aggregate_expressions``) bound to the two sides, as
    ``expression_operand`` binds a computed column; every decline names the aggregate's own case."""
    if holds_distance(it.expr):
        raise decline("DISTANCE inside an aggregate over an expression")
    if _string_valued(it.expr):
        raise decline("aggregate over a string-valued expression")

    def bind(o) -> Operand:
        if o[0] == "lit":
            v = o[1]
            return Operand("str" if isinstance(v, str) else ("float" if isinstance(v, float) else "int"), v)
        ref: ColRef = o[1]
        if ref.star:
            raise decline("star in an expression inside an aggregate")
        return Operand(_side_of(ref, left, right, "an aggregate argument"), ref.column)

    op = bind_expression(it.expr, bind)
    if not operand_sides(op):
        raise decline("aggregate over a constant expression")
    nodes, depth = expression_cost(op)
    if depth > MAX_EXPR_DEPTH:
        raise decline(f"aggregate over an expression too deep for the kernel ({depth} values live, at most {MAX_EXPR_DEPTH})")
    if nodes > MAX_EXPR_NODES:
        raise decline(f"aggregate over an expression too large for one call ({nodes} nodes, at most {MAX_EXPR_NODES})")
    return op


def check_expression_sizes(residuals, kind: str) -> None:
    """Decline (never a run-time error) a condition whose arithmetic one select call cannot hold: an operand deeper
    than ``MAX_EXPR_DEPTH``, or more than ``MAX_EXPR_NODES`` nodes among the residuals ``execute()`` evaluates in
    one call -- those reading the same tables (left only: before the join; right only; both: on the pairs), and
    for SEMI / ANTI the WHERE residuals on their own."""
    per_call: dict = {}
    for r in residuals:
        nodes = 0
        for o in (r.lhs, r.rhs):
            n, d = expression_cost(o)
            if d > MAX_EXPR_DEPTH:
                raise decline(f"expression too deep for the select kernel ({d} values live, at most {MAX_EXPR_DEPTH})")
            nodes += n
        sides = frozenset(operand_sides(r.lhs) | operand_sides(r.rhs))
        call = ("where" if kind in ("SEMI", "ANTI") and r.clause == "where" else "on", sides)
        if kind == "LEFT" and r.clause == "where":
            call = ("where", None)      # the WHERE of a LEFT plan filters the padded result in one call per half
        per_call[call] = per_call.get(call, 0) + nodes
        if per_call[call] > MAX_EXPR_NODES:
            raise decline(f"expressions too large for one select call ({per_call[call]} nodes, at most {MAX_EXPR_NODES})")


def resolve_residuals(clause_terms, left: PlanSide, right: PlanSide, kind: str) -> tuple:
    """``[(clause, term)]`` -> residuals.  A term is a comparison ``("cmp", lhs, op, rhs)`` or
    a disjunction ``("or", [cmp, ...])``; the members of one disjunction share a fresh group id."""
    out, group = [], 0
    for clause, t in clause_terms:
        if t[0] == "or":
            group += 1
            out.extend(resolve_residual(clause, leaf, left, right, kind, group) for leaf in t[1])
        elif t[0] == "tree":    # a nested condition as one boolean program: kept when it IS TRUE
            out.append(resolve_residual(clause, ("cmp", t[1], "istrue", ("lit", 0)), left, right, kind))
        else:
            out.append(resolve_residual(clause, t, left, right, kind))
    check_expression_sizes(out, kind)
    return tuple(out)


def resolve_residual(clause: str, term, left: PlanSide, right: PlanSide, kind: str, group: int = 0) -> Residual:
    """Bind a comparison's operands to the two sides; qualifier mistakes are user
    errors, as in ``_validate_extra_qualifiers`` (intersects_duckdb.py:914-959)."""
    _, lhs, op, rhs = term

    def bind(o) -> Operand:
        if o[0] == "lit":
            v = o[1]
            return Operand("str" if isinstance(v, str) else ("float" if isinstance(v, float) else "int"), v)
        ref: ColRef = o[1]
        if ref.star:
            raise decline("star in a join condition")
        if ref.table is None:
            raise ValueError(
                f"dialect='hip' cannot inline the extra predicate: column {ref.column!r} must be "
                f"qualified with {left.alias!r} or {right.alias!r}")
        q = norm(ref.table, ref.table_quoted)
        if q == left.alias:
            return Operand("l", ref.column)
        if q == right.alias:
            if kind in ("SEMI", "ANTI") and clause == "where":
                raise ValueError(f"{kind} join: the WHERE clause cannot reference the right side "
                                 f"({ref.table}.{ref.column})")
            return Operand("r", ref.column)
        raise ValueError(f"dialect='hip' cannot inline the extra predicate: unknown table qualifier "
                         f"{ref.table!r}; expected {left.alias!r} or {right.alias!r}")

    a, b = bind_expression(lhs, bind), bind_expression(rhs, bind)
    if not operand_sides(a) and not operand_sides(b):
        raise decline("constant predicate in the join condition")
    return Residual(clause, a, op, b, group)


def resolve_count_projection(items, group_cols, left: PlanSide, right: PlanSide):
    """The count_overlaps projection: left key columns + ONE aliased COUNT(<right col>);
    GROUP BY must be exactly the projected left columns (intersects_duckdb.py:484-539)."""
    out = []
    n_count = 0
    keys = set()
    for it in items:
        ref = it.ref
        is_count = it.func == "COUNT" or (ref is not None and ref.count)
        if it.func not in (None, "COUNT") or it.distinct:
            raise decline("count_overlaps with an aggregate other than COUNT(<right column>)")
        if ref is None or ref.star or ref.table is None:
            raise decline("count_overlaps projection that is not a qualified column")
        q = norm(ref.table, ref.table_quoted)
        if is_count:
            n_count += 1
            if q != right.alias:
                raise decline("COUNT over a left-side column")
            if not it.alias:
                raise decline("count_overlaps COUNT without an alias")
            out.append(Projection("count", ref.column, it.alias))
        else:
            if q != left.alias:
                raise decline("count_overlaps key from the right side")
            keys.add(ref.column)
            out.append(Projection("l", ref.column, it.alias or ref.column))
    if n_count != 1 or not keys:
        raise decline("count_overlaps needs left key columns and exactly one COUNT")
    gkeys = set()
    for g in group_cols:
        if g.table is None or norm(g.table, g.table_quoted) != left.alias:
            raise decline("GROUP BY column that is not a left-side qualified column")
        gkeys.add(g.column)
    if gkeys != keys:
        raise decline("GROUP BY keys differ from the projected left columns")
    names = [p.name for p in out]
    if len(set(names)) != len(names):
        raise decline("duplicate output names in count_overlaps")
    return tuple(out)


def _resolve_grouped(shape: JoinShape, left: PlanSide, right: PlanSide, left_only: bool, exprs_out: list | None = None):
    """Projection with plain aggregates and / or a GROUP BY: key columns + aggregates, finished on
    the projected table (the reference rebuilds them over the wrapper relation,
    intersects_duckdb.py:1402-1644).  Returns (projection, aggregates, group names)."""
    proj: list[Projection] = []
    aggs: list[Aggregate] = []
    names: list[str] = []
    key_names: dict[tuple[str, str], str] = {}
    for i, it in enumerate(shape.items):
        ref = it.ref
        if it.func is None:
            if ref.star:
                raise decline("star projection")
            side = _side_of(ref, left, right, "the SELECT list")
            if side == "r" and left_only:
                raise ValueError(f"Column {ref.table}.{ref.column} references the right side of a SEMI/ANTI join "
                                 "(left-side columns only)")
            name = it.alias or ref.column
            proj.append(Projection(side, ref.column, name))
            key_names[(side, ref.column)] = name
            names.append(name)
            continue
        if it.func not in AGG_FUNCS:
            raise decline(f"aggregate {it.func}")
        if it.distinct and it.func != "COUNT":
            raise decline(f"{it.func}(DISTINCT ...)")
        if it.expr is not None:               # an aggregate over an expression: the tree goes to the plan's expressions
            bound = aggregate_operand(it, left, right)
            if bound not in exprs_out:
                exprs_out.append(bound)
            side, column = "x", str(exprs_out.index(bound))
        elif ref is None:                     # COUNT(*)
            if it.func != "COUNT":
                raise decline(f"{it.func}(*)")
            side, column = "*", "*"
        else:
            if ref.star:
                raise decline("star inside an aggregate")   # #204
            side = _side_of(ref, left, right, "an aggregate argument")
            if side == "r" and left_only:
                raise ValueError(f"Column {ref.table}.{ref.column} references the right side of a SEMI/ANTI join "
                                 "(left-side columns only)")
            column = ref.column
        name = it.alias or f"{it.func.lower()}_{i}"
        aggs.append(Aggregate(it.func, side, column, name, it.distinct))
        names.append(name)
    if len(set(names)) != len(names):
        raise decline("duplicate output names")
    groups: list[str] = []
    for g in shape.group_by:
        side = _side_of(g, left, right, "GROUP BY")
        if side == "r" and left_only:
            raise ValueError(f"Column {g.table}.{g.column} references the right side of a SEMI/ANTI join")
        if (side, g.column) not in key_names:
            # a key that is not projected still groups: carried as a hidden column
            hidden = f"__giql_g{len(groups)}"
            proj.append(Projection(side, g.column, hidden))
            key_names[(side, g.column)] = hidden
        groups.append(key_names[(side, g.column)])
    plain = [p for p in proj if not p.name.startswith("__giql_g")]
    if aggs and any(p.name not in groups for p in plain):
        raise ValueError("a projected column must appear in GROUP BY or inside an aggregate")
    if not aggs and shape.group_by and any(p.name not in groups for p in plain):
        raise ValueError("a projected column must appear in GROUP BY or inside an aggregate")
    return tuple(proj), tuple(aggs), tuple(groups), tuple(names)


def _resolve_having(shape: JoinShape, proj, aggs, left: PlanSide, right: PlanSide, left_only: bool):
    """HAVING conjuncts -> comparisons over the grouped result's columns.  An aggregate that the SELECT
    list does not hold is added as a hidden ``__giql_h<n>`` aggregate (dropped from the output); a column
    must be a grouping key (by its qualified name or its output name).  Returns (aggregates, having)."""
    aggs = list(aggs)
    by_col = {(p.side, p.column): p.name for p in proj}
    out_names = {p.name for p in proj if not p.name.startswith("__giql_")} | {a.name for a in aggs}
    having: list[Having] = []

    def bind(o) -> Operand:
        if o[0] == "lit":
            v = o[1]
            return Operand("str" if isinstance(v, str) else ("float" if isinstance(v, float) else "int"), v)
        if o[0] == "col":
            ref: ColRef = o[1]
            if ref.star:
                raise decline("star in HAVING")
            if ref.table is None:
                if ref.column in out_names:
                    return Operand("name", ref.column)
                raise ValueError(f"HAVING {ref.column!r}: not an output column; qualify it with a table alias")
            side = _side_of(ref, left, right, "HAVING")
            name = by_col.get((side, ref.column))
            if name is None:
                raise ValueError(f"HAVING {ref.table}.{ref.column}: the column must appear in GROUP BY "
                                 "or inside an aggregate")
            return Operand("name", name)
        if o[0] == "fn":
            raise decline("arithmetic in HAVING")
        it: SelItem = o[1]
        if it.func not in AGG_FUNCS:
            raise decline(f"aggregate {it.func}")
        if it.distinct and it.func != "COUNT":
            raise decline(f"{it.func}(DISTINCT ...)")
        if it.ref is None:
            if it.func != "COUNT":
                raise decline(f"{it.func}(*)")
            side, column = "*", "*"
        else:
            if it.ref.star:
                raise decline("star inside an aggregate")
            side = _side_of(it.ref, left, right, "an aggregate argument")
            if side == "r" and left_only:
                raise ValueError(f"Column {it.ref.table}.{it.ref.column} references the right side of a SEMI/ANTI join "
                                 "(left-side columns only)")
            column = it.ref.column
        for a in aggs:
            if (a.func, a.side, a.column, a.distinct) == (it.func, side, column, it.distinct):
                return Operand("name", a.name)
        hidden = Aggregate(it.func, side, column, f"__giql_h{sum(a.name.startswith('__giql_h') for a in aggs)}",
                           it.distinct)
        aggs.append(hidden)
        return Operand("name", hidden.name)

    group = 0
    for term in shape.having:
        leaves, g = [term], 0
        if term[0] == "or":
            group += 1
            leaves, g = term[1], group
        for _tag, lhs, op, rhs in leaves:
            a, b = bind(lhs), bind(rhs)
            if a.kind != "name" and b.kind != "name":
                raise decline("constant HAVING predicate")
            having.append(Having(a, op, b, g))
    return tuple(aggs), tuple(having)


def _resolve_order(shape: JoinShape, proj, aggs, left: PlanSide, right: PlanSide, left_only: bool, grouped: bool):
    """ORDER BY keys -> output column names; a qualified column that is not projected rides along as
    a hidden column (dropped after the sort).  Returns (extra hidden projections, order spec)."""
    out_names = [p.name for p in proj] + [a.name for a in aggs]
    by_col = {(p.side, p.column): p.name for p in proj}
    hidden: list[Projection] = []
    order: list[tuple[str, bool, bool]] = []
    for k in shape.order_by:
        nulls_first = (not k.desc) if k.nulls_first is None else bool(k.nulls_first)
        ref = k.ref
        if ref.star:
            raise decline("ORDER BY *")
        if ref.table is None:
            if ref.column in out_names:        # an output name (alias)
                order.append((ref.column, k.desc, nulls_first))
                continue
            raise ValueError(f"ORDER BY {ref.column!r}: not an output column; qualify it with a table alias")
        side = _side_of(ref, left, right, "ORDER BY")
        if side == "r" and left_only:
            raise ValueError(f"ORDER BY {ref.table}.{ref.column} references the right side of a SEMI/ANTI join")
        name = by_col.get((side, ref.column))
        if name is None:
            if grouped or shape.distinct:
                raise decline("ORDER BY a column that is neither projected nor grouped")
            name = f"__giql_o{len(hidden)}"
            hidden.append(Projection(side, ref.column, name))
            by_col[(side, ref.column)] = name
        order.append((name, k.desc, nulls_first))
    return tuple(hidden), tuple(order)


#: aggregates of one map-shape plan, hidden HAVING aggregates included (``GIQL_PAIR_AGG_MAX``)
MAP_AGG_MAX = 8


def _is_qualified(ref, alias: str) -> bool:
    return ref is not None and not ref.star and ref.table is not None and norm(ref.table, ref.table_quoted) == alias


def map_aggregate_ok(func: str, side: str, distinct: bool) -> bool:
    """An aggregate the map shape computes per left row: ``COUNT(*)``, ``COUNT(<right column>)``, or SUM / AVG / MIN /
    MAX of a right-side column, without DISTINCT (the column's type is execute()'s to check: the plan has no schema);
    side "x": any of the five over an expression of the pair (the ``aggregate_expressions`` opt-in)."""
    if distinct:
        return False
    if side == "x":     # an expression over the pair (``aggregate_expressions``): its type is the tree's
        return func in ("COUNT", "SUM", "AVG", "MIN", "MAX")
    return (func == "COUNT" and side in ("*", "r")) or (func in ("SUM", "AVG", "MIN", "MAX") and side == "r")


def is_map_shape(shape: JoinShape, left: PlanSide, right: PlanSide) -> bool:
    """The routing decision of the ``join_aggregates`` opt-in, on the parsed shape alone (bedtools ``map``): an INNER
    join, or a LEFT join with its spatial predicate in ON and no WHERE, grouped by qualified left-side columns only,
    every projected plain column a group key, and 1..8 aliased aggregates over the right side (map_aggregate_ok).  A
    lone ``COUNT(b.col)`` under a bare LEFT ... ON is the count_overlaps shape and stays with it."""
    if not shape.join_aggregates or shape.kind not in ("INNER", "LEFT") or left.alias == right.alias:
        return False
    cmp_terms = [t for t in list(shape.on_terms) + list(shape.where_terms) if t[0] not in JOIN_TERMS]
    if shape.kind == "LEFT" and (shape.where_terms or not any(t[0] in JOIN_TERMS for t in shape.on_terms)):
        return False
    if not shape.group_by or not all(_is_qualified(g, left.alias) for g in shape.group_by):
        return False
    keys = {g.column for g in shape.group_by}
    aggs = []
    for it in shape.items:
        if it.distance is not None or (it.expr is not None and (it.func is None or not shape.aggregate_expressions)):
            return False
        if it.func is None:
            if not _is_qualified(it.ref, left.alias) or it.ref.count or it.ref.column not in keys:
                return False
            continue
        if it.func not in AGG_FUNCS or not it.alias:
            return False
        if it.expr is not None:
            side = "x"
        elif it.ref is None:
            side = "*"
        elif _is_qualified(it.ref, right.alias):
            side = "r"
        else:
            return False
        if not map_aggregate_ok(it.func, side, it.distinct):
            return False
        aggs.append((it.func, side))
    if not 1 <= len(aggs) <= MAP_AGG_MAX:
        return False
    if shape.kind == "LEFT" and aggs == [("COUNT", "r")] and not cmp_terms:
        return False   # count_overlaps
    return True


# ------------------------------------------------------------------- the gate
def lower_join_shape(shape: JoinShape, tables: Tables) -> JoinPlan:
    """:class:`JoinShape` -> :class:`JoinPlan`, or :class:`HipDeclined` / ``ValueError``."""
    kind = shape.kind
    items = shape.items
    if shape.sides is not None:
        left, right = shape.sides
    else:
        left = table_side(shape.from_ref, tables)
        right = table_side(shape.join_ref, tables)
    has_count_item = any((it.func == "COUNT" and it.ref is not None and not it.distinct) for it in items)
    # the ``join_aggregates`` opt-in: a LEFT join in the map shape is neither count_overlaps nor in need of
    # ``outer_joins`` -- its aggregates are computed per left row, no padded pair is ever produced
    map_shape = is_map_shape(shape, left, right)
    dist_items = [it for it in items if it.distance is not None]
    if dist_items and kind != "INNER":
        # the value is defined per PAIR: SEMI / ANTI keep left rows, count_overlaps counts them
        raise decline(f"{'count_overlaps / outer' if kind == 'LEFT' else kind} join with a DISTANCE in the SELECT list")
    if dist_items and (shape.group_by or shape.having or any(it.func is not None for it in items)):
        raise decline("DISTANCE in the SELECT list beside GROUP BY / HAVING / aggregates")
    if any(it.expr is not None and it.func is not None for it in items) and not map_shape:
        raise decline("aggregate over an expression outside the map shape (an INNER join, or a LEFT join with its "
                      "predicate in ON and no WHERE; GROUP BY qualified left-side columns; 1 to 8 aliased aggregates)")
    expr_items = [it for it in items if it.expr is not None and it.func is None]
    if expr_items and (shape.group_by or shape.having or any(it.func is not None for it in items)):
        raise decline("expression in the SELECT list beside GROUP BY / HAVING / aggregates")
    if kind == "LEFT":
        # count_overlaps: LEFT [OUTER] JOIN ... COUNT(b.col) ... GROUP BY left keys
        # (_match_count_overlaps, intersects_duckdb.py:432-548); every other outer join declines (:661-662)
        # unless the caller opted in (JoinShape.outer_joins): then it is a LEFT plan
        if has_count_item and not map_shape:
            kind = "COUNT"
        elif not shape.outer_joins and not map_shape:
            raise decline("LEFT outer join")
    if kind == "COUNT" and not shape.on_seen:
        raise decline("count_overlaps without an ON clause")
    if shape.using:
        # the single-column form whose column is both tables' chrom column: the per-chromosome
        # partition IS that equi-join (intersects_duckdb.py:727-735, 1190-1201)
        if len(shape.using) != 1:
            raise decline("multi-column USING")
        u = shape.using[0].casefold()
        if left.chrom_col.casefold() != right.chrom_col.casefold() or left.chrom_col.casefold() != u:
            raise decline("USING on a column that is not both tables' chromosome column")
    on_terms, where_terms = list(shape.on_terms), list(shape.where_terms)
    if not shape.on_seen and not shape.using and kind in ("SEMI", "ANTI"):
        raise decline("SEMI/ANTI join with its INTERSECTS outside ON")  # #201
    spatial = [t for t in on_terms + where_terms if t[0] in JOIN_TERMS]
    if not spatial:
        raise decline("join without an INTERSECTS predicate")
    if len(spatial) > 1:
        raise decline("more than one INTERSECTS" if all(t[0] == "intersects" for t in spatial)
                      else "more than one spatial predicate in a join")
    if kind == "LEFT" and not any(t[0] in JOIN_TERMS for t in on_terms):
        # in WHERE the predicate would filter the padded rows away again: an INNER join written the long way
        raise decline("LEFT join with its spatial predicate outside ON")
    predicate, lhs, rhs = spatial[0][:3]
    max_distance = spatial[0][3] if predicate == DISTANCE_TERM else None
    if kind == "LEFT" and (predicate == "intersects" or shape.row_predicates):
        # bedtools -v: LEFT JOIN ... WHERE b.<chrom | start | end> IS NULL with no other use of the right table is
        # the ANTI join (a matched row's right key columns are never NULL) -- semi_anti, not pairs thrown away
        rest = _anti_shortcut(shape, where_terms, right)
        if rest is not None:
            kind, where_terms = "ANTI", rest
    if expr_items and kind not in ("INNER", "LEFT"):
        # the value is defined per PAIR (or padded row): SEMI / ANTI keep left rows
        raise decline(f"{kind} join with an expression in the SELECT list")
    label = "DISTANCE" if predicate == DISTANCE_TERM else predicate.upper()
    row_pred = predicate != "intersects" and shape.row_predicates and kind in ("SEMI", "ANTI", "COUNT")
    if predicate != "intersects" and not shape.row_predicates:
        # CONTAINS / WITHIN / DISTANCE <= N run as the pair-producing join only (HipEngine.contain_join / window_join)
        # unless the caller opted in (JoinShape.row_predicates): HipEngine.semi_anti_pred / count_pred
        if kind in ("SEMI", "ANTI"):
            raise decline(f"{kind} join over {label}")
        if kind == "COUNT":
            raise decline(f"count_overlaps over {label}")
    if kind in ("SEMI", "ANTI") and not any(t[0] == "intersects" or (row_pred and t[0] in JOIN_TERMS) for t in on_terms):
        raise decline("SEMI/ANTI join with its INTERSECTS outside ON")  # #201
    cmp_terms = ([("on", t) for t in on_terms if t[0] in ("cmp", "or", "tree")]
                 + [("where", t) for t in where_terms if t[0] in ("cmp", "or", "tree")])
    if kind == "COUNT" and (cmp_terms or where_terms):
        raise decline("count_overlaps with predicates beside the INTERSECTS")  # bare ON only (:432-548)
    if kind == "COUNT" and not shape.group_by:
        raise decline("count_overlaps without GROUP BY")

    for side_ref in (lhs, rhs):
        if side_ref.table is None or side_ref.star:
            raise decline("INTERSECTS operand that is not a table-qualified column")
    la, ra = norm(lhs.table, lhs.table_quoted), norm(rhs.table, rhs.table_quoted)
    if left.alias == right.alias:
        raise decline("same alias on both sides")
    if left.table == right.table:
        raise decline("self-join")
    # FROM-side orientation swap (intersects_duckdb.py:359-410)
    if la == left.alias and ra == right.alias:
        l_col, r_col = lhs.column, rhs.column
    elif ra == left.alias and la == right.alias:
        l_col, r_col = rhs.column, lhs.column
        predicate = _FLIPPED[predicate]     # the plan states it as left <predicate> right
    else:
        raise decline("INTERSECTS operands that do not name the two joined tables")
    if l_col != genomic_col(left.table, tables) or r_col != genomic_col(right.table, tables):
        raise ValueError(
            f"{'DISTANCE' if spatial[0][0] == DISTANCE_TERM else spatial[0][0].upper()} operands must be the tables' genomic columns "
            f"({genomic_col(left.table, tables)!r} / {genomic_col(right.table, tables)!r})")
    if kind == "COUNT":
        if shape.distinct:
            raise decline("DISTINCT with count_overlaps")
        if shape.order_by or shape.limit is not None or shape.offset is not None or shape.having:
            raise decline("HAVING / ORDER BY / LIMIT over count_overlaps")
        return JoinPlan("COUNT", left, right, resolve_count_projection(items, shape.group_by, left, right),
                        max_distance=max_distance if row_pred else None, predicate=predicate, row_predicates=row_pred)

    left_only = kind in ("SEMI", "ANTI")
    grouped = bool(shape.group_by) or any(it.func is not None for it in items) or bool(shape.having)
    output: tuple[str, ...] = ()
    having: tuple[Having, ...] = ()
    strands: list = []          # strand columns of the stranded DISTANCE select items (all alike: one pair of tables)
    exprs: list = []            # the computed columns, as their projections number them
    # a.* / b.* lower only beside a computed column of an opted-in pair plan, and not under DISTINCT (the two tables'
    # columns may share names, which a DISTINCT by output name cannot tell apart)
    stars = bool(expr_items) and kind in ("INNER", "LEFT") and not shape.distinct
    if grouped:
        proj, aggs, groups, output = _resolve_grouped(shape, left, right, left_only, exprs_out=exprs)
        visible_aggs = aggs
        aggs, having = _resolve_having(shape, proj, aggs, left, right, left_only)
        if not visible_aggs and not groups and aggs:
            # HAVING over the whole result as ONE group, nothing aggregated in the SELECT list: the plain
            # columns it projects are neither grouped nor aggregated
            raise ValueError("a projected column must appear in GROUP BY or inside an aggregate")
        if map_shape and not (len(aggs) <= MAP_AGG_MAX and all(map_aggregate_ok(a.func, a.side, a.distinct) for a in aggs)):
            # an aggregate that only HAVING names falls outside the shape: the query lowers as it does without the flag
            from dataclasses import replace

            return lower_join_shape(replace(shape, join_aggregates=False), tables)
    else:
        proj, aggs, groups = resolve_projection(items, left, right, left_only, tables=tables, strands_out=strands,
                                                exprs_out=exprs, stars=stars), (), ()
        visible_aggs = ()
    hidden, order = _resolve_order(shape, proj, visible_aggs, left, right, left_only, grouped)
    if predicate == DISTANCE_TERM:
        # x.chrom = y.chrom beside the predicate (the documented recipe writes it): a NULL distance already drops
        # pairs across chromosomes, the join IS per chromosome -- absorbed, not run as a string comparison per pair
        # (in the WHERE of a LEFT join the equality is a filter of its own: it drops the padded rows)
        cmp_terms = [(c, t) for c, t in cmp_terms
                     if (kind == "LEFT" and c == "where") or not _is_chrom_equality(t, left, right)]
    residuals = resolve_residuals(cmp_terms, left, right, kind)
    strand_col = strands[0] if strands else None
    return JoinPlan(kind, left, right, tuple(proj) + hidden, shape.distinct, max_distance=max_distance,
                    residuals=residuals, strand_col=strand_col,
                    aggregates=aggs, group_by=groups, having=having, order_by=order,
                    limit=shape.limit, offset=shape.offset, output=output, predicate=predicate,
                    row_predicates=row_pred, expressions=tuple(exprs), join_aggregates=map_shape)


def _col_refs(x):
    """Every :class:`ColRef` inside a term, an operand, a select item or a list of them."""
    if isinstance(x, ColRef):
        yield x
    elif isinstance(x, SelItem):
        yield from _col_refs(x.ref)
        yield from _col_refs(x.distance)
        yield from _col_refs(x.expr)
    elif isinstance(x, OrderKey):
        yield from _col_refs(x.ref)
    elif isinstance(x, (tuple, list)):
        for y in x:
            yield from _col_refs(y)


def _anti_shortcut(shape: JoinShape, where_terms: list, right: PlanSide):
    """The WHERE terms left over when a LEFT join is an ANTI join in disguise, else None: one conjunct is
    ``<right>.<chrom | start | end column> IS NULL`` and nothing else in the statement -- the SELECT list, the other
    WHERE conjuncts, GROUP BY, HAVING, ORDER BY -- reads the right table (a star counts as reading it)."""
    def reads_right(x) -> bool:
        return any(r.star or (r.table is not None and norm(r.table, r.table_quoted) == right.alias)
                   for r in _col_refs(x))

    keys = (right.chrom_col, right.start_col, right.end_col)
    for i, t in enumerate(where_terms):
        if (t[0] == "cmp" and t[2] == "isnull" and t[1][0] == "col" and isinstance(t[1][1], ColRef)
                and not t[1][1].star and t[1][1].column in keys and reads_right(t[1])):
            rest = where_terms[:i] + where_terms[i + 1:]
            if not reads_right([shape.items, rest, shape.group_by, shape.having, shape.order_by]):
                return rest
            return None
    return None


def _is_chrom_equality(term, left: PlanSide, right: PlanSide) -> bool:
    """``<left alias>.<its chrom column> = <right alias>.<its chrom column>`` (either way round)."""
    if term[0] != "cmp" or term[2] != "=" or term[1][0] != "col" or term[3][0] != "col":
        return False
    got = set()
    for o in (term[1], term[3]):
        ref: ColRef = o[1]
        if ref.table is None or ref.star:
            return False
        q = norm(ref.table, ref.table_quoted)
        for tag, side in (("l", left), ("r", right)):
            if q == side.alias and ref.column == side.chrom_col:
                got.add(tag)
    return got == {"l", "r"}


# ------------------------------------------------------------------ DISJOIN
DISJOIN_RESERVED_PREFIX = "__giql_dj_"   # the reference's CTE names (src/giql/constants.py DJ_PREFIX; disjoin.py:147-178)


@dataclass
class DisjoinShape:
    """What either front end hands to :func:`lower_disjoin_shape`: ``SELECT ... FROM DISJOIN(target
    [, reference := ref]) [alias]`` with the clauses of the outer SELECT."""

    items: list[SelItem]
    target: TableRef
    reference: TableRef | None = None          # None: self mode
    alias: str | None = None                   # the table function's alias (qualifies output columns)
    distinct: bool = False
    where: bool = False                        # clauses the lowering cannot express: seen, then declined
    group_by: bool = False
    having: bool = False
    order_by: list[OrderKey] = field(default_factory=list)
    limit: int | None = None
    offset: int | None = None
    sides: tuple[PlanSide, PlanSide | None] | None = None   # as resolved by the caller (the plugin), else from ``tables``
    # the GROUP BY column list, where the front end read it (the text front end under ``disjoin_aggregates``); None:
    # only seen (``group_by``), and declined
    group_cols: list[ColRef] | None = None


def lower_disjoin_shape(shape: DisjoinShape, tables: Tables, disjoin_aggregates: bool = False) -> JoinPlan:
    """The gate of DISJOIN, shared by both front ends (src/giql/expanders/disjoin.py:102-202): projections over
    the target's columns and the three ``disjoin_*`` columns, DISTINCT, ORDER BY output names, LIMIT / OFFSET.
    WHERE, GROUP BY / aggregates and HAVING over the operator's rows decline.

    ``disjoin_aggregates``: in self mode, ``GROUP BY`` the three ``disjoin_*`` columns with ``COUNT(*) AS <alias>``
    lowers to a plan answered from the coverage segments (``segments="depth"``,
    docs/recipes/clustering.rst "Reconstruct disjoin() Coverage Segments"), and ``SELECT DISTINCT`` over exactly
    the three columns is marked ``segments="distinct"`` (docs/recipes/disjoin.rst "Build a Disjoint Partition")."""
    names = [shape.target.name] + ([shape.reference.name] if shape.reference is not None else [])
    for n in names + ([shape.alias] if shape.alias else []):
        if n.casefold().startswith(DISJOIN_RESERVED_PREFIX):
            raise decline(f"the name {n!r} uses the reserved prefix {DISJOIN_RESERVED_PREFIX!r} of DISJOIN")
    if shape.where:
        raise decline("WHERE over the rows of DISJOIN")
    grouped = shape.group_by or any(it.func is not None or (it.ref is not None and it.ref.count) for it in shape.items)
    if grouped and not (disjoin_aggregates and shape.group_cols is not None):
        raise decline("GROUP BY / aggregates over the rows of DISJOIN")
    if shape.having:
        raise decline("HAVING over the rows of DISJOIN")
    if grouped and shape.reference is not None:
        raise decline("GROUP BY over DISJOIN with reference := (the coverage segments are those of self mode)")
    if shape.sides is not None:
        left, right = shape.sides
    else:
        left = table_side(shape.target, tables)
        right = table_side(shape.reference, tables) if shape.reference is not None else None
    qualifiers = {norm(shape.alias)} if shape.alias else {left.alias}

    def own(ref: ColRef, where: str) -> str:
        if ref.table is not None and norm(ref.table, ref.table_quoted) not in qualifiers:
            raise ValueError(f"Unknown table qualifier {ref.table!r} in {where}")
        return ref.column

    if grouped:
        return _lower_disjoin_depth(shape, left, own)
    proj, out_names = [], []
    for it in shape.items:
        ref = it.ref
        if ref.star:
            own(ref, "the SELECT list")
            if it.alias:
                raise decline("aliased star projection")
            proj.append(Projection("star", "*", "*"))
            out_names.append(None)
            continue
        column = own(ref, "the SELECT list")
        if column.casefold().startswith(DISJOIN_RESERVED_PREFIX):
            raise decline(f"the name {column!r} uses the reserved prefix {DISJOIN_RESERVED_PREFIX!r} of DISJOIN")
        name = it.alias or column
        proj.append(Projection("disjoin" if column in DISJOIN_COLUMNS else "l", column, name))
        out_names.append(name)
    if not proj:
        raise decline("empty SELECT list")
    has_star = any(p.side == "star" for p in proj)
    order = []
    for o in shape.order_by:
        name = own(o.ref, "ORDER BY")
        if name not in out_names and not has_star:
            if shape.distinct:
                raise ValueError("ORDER BY a column that DISTINCT does not keep")
            # carried for the sort only, dropped from the result (the "__giql_" convention of the join plans)
            hidden = f"__giql_o{len(order)}"
            proj.append(Projection("disjoin" if name in DISJOIN_COLUMNS else "l", name, hidden))
            name = hidden
        nulls_first = o.nulls_first if o.nulls_first is not None else not o.desc
        order.append((name, o.desc, nulls_first))
    # DISTINCT over exactly the three appended columns is the set of coverage segments, whatever their depth
    segments = None
    if disjoin_aggregates and shape.distinct and right is None \
            and all(p.side == "disjoin" for p in proj) and sorted(p.column for p in proj) == sorted(DISJOIN_COLUMNS):
        segments = "distinct"
    return JoinPlan("DISJOIN", left, right, tuple(proj), shape.distinct, order_by=tuple(order), limit=shape.limit,
                    offset=shape.offset, segments=segments)


def _lower_disjoin_depth(shape: DisjoinShape, left: PlanSide, own) -> JoinPlan:
    """``SELECT <disjoin_* columns, COUNT(*) AS alias> FROM DISJOIN(t) GROUP BY`` the three ``disjoin_*`` columns:
    one row per coverage segment with the number of target rows over it (``segments="depth"``)."""
    if shape.distinct:
        raise decline("DISTINCT beside GROUP BY over DISJOIN")
    keys = [own(ref, "GROUP BY") for ref in shape.group_cols]
    if any(ref.star for ref in shape.group_cols) or sorted(keys) != sorted(DISJOIN_COLUMNS):
        raise decline("GROUP BY over DISJOIN other than exactly disjoin_chrom, disjoin_start, disjoin_end")
    proj, out_names = [], []
    for it in shape.items:
        if it.distance is not None or it.expr is not None:
            raise decline("expression in the SELECT list of a grouped DISJOIN")
        if it.func is not None:
            if it.func != "COUNT" or it.distinct:
                raise decline(f"{it.func}({'DISTINCT ' if it.distinct else ''}...) over the rows of DISJOIN: only "
                              "COUNT(*) is computed per segment")
            if it.ref is not None:
                raise decline(f"COUNT({it.ref.column}) over the rows of DISJOIN: only COUNT(*) is computed per segment")
            if not it.alias:
                raise decline("COUNT(*) without an alias over the rows of DISJOIN")
            proj.append(Projection("count", "*", it.alias))
            out_names.append(it.alias)
            continue
        if it.ref.star:
            raise decline("star projection beside GROUP BY over DISJOIN")
        column = own(it.ref, "the SELECT list")
        if column not in DISJOIN_COLUMNS:
            raise decline(f"target column {column!r} beside GROUP BY over DISJOIN (it is not a GROUP BY key)")
        proj.append(Projection("disjoin", column, it.alias or column))
        out_names.append(it.alias or column)
    if not proj:
        raise decline("empty SELECT list")
    if len(set(out_names)) != len(out_names):
        raise decline("two output columns of one name over a grouped DISJOIN")
    order = []
    for o in shape.order_by:
        name = own(o.ref, "ORDER BY")
        if name not in out_names:
            if name not in DISJOIN_COLUMNS:
                raise decline(f"ORDER BY {name!r}: not an output name or GROUP BY key of the grouped DISJOIN")
            hidden = f"__giql_o{len(order)}"     # carried for the sort only, as the ungrouped plan does
            proj.append(Projection("disjoin", name, hidden))
            name = hidden
        nulls_first = o.nulls_first if o.nulls_first is not None else not o.desc
        order.append((name, o.desc, nulls_first))
    return JoinPlan("DISJOIN", left, None, tuple(proj), False, order_by=tuple(order), limit=shape.limit,
                    offset=shape.offset, segments="depth")
