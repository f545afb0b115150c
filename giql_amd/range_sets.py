"""Literal genomic ranges and quantified sets of them: ``interval INTERSECTS | CONTAINS | WITHIN 'chr1:1000-2000'``,
``... ANY(...)`` / ``SOME(...)`` / ``ALL(...)`` and their negations over ONE table (docs/dialect/quantifiers.rst).

The reference expands such a predicate to one term per range, ``chrom = c AND <cmp on start> AND <cmp on end>``
over the canonicalised column (``start + so``, ``end + eo``), OR-ed for ANY and AND-ed for ALL
(src/giql/expanders/intersects.py:85-133, 243-270).  Here the offsets move onto the literal -- ``start + so < hi``
is ``start < hi - so`` -- so the raw columns are compared as they lie in memory and nothing can wrap at the ends of
int32; the moved bounds are int64.  What collapses to comparisons is folded into the residuals the select kernel
evaluates (:func:`fold`); ANY over two or more ranges is left to ``HipEngine.range_set_any``.  sqlglot-free.
"""

from __future__ import annotations

import re

from .plan import Operand, PlanSide, RangeSet, Residual

#: (so, eo): ``start + so`` / ``end + eo`` is the canonical 0-based half-open position of a table's raw coordinate --
#: the offsets ``DeviceSide`` applies for joins (``engine.ENCODING_OFFSETS``)
CANONICAL_OFFSETS = {
    ("0based", "half_open"): (0, 0),
    ("0based", "closed"): (0, +1),
    ("1based", "half_open"): (-1, -1),
    ("1based", "closed"): (-1, 0),
}

#: sets per query and ranges per set that reach the kernel (``GIQL_RANGE_MAX_SETS`` / ``GIQL_RANGE_MAX_RANGES``); the
#: reference's own note sends larger sets to a table and a JOIN (docs/dialect/quantifiers.rst:115)
MAX_KERNEL_SETS = 8
MAX_SET_RANGES = 1024

_POINT = re.compile(r"^(?P<chrom>[\w.]+):(?P<pos>\d+)$")
_BRACKETED = re.compile(r"^(?P<chrom>[\w.]+):\[(?P<start>\d+),(?P<end>\d+)(?P<close>[)\]])(?::[+-])?$")
_DASHED = re.compile(r"^(?P<chrom>[\w.]+):(?P<start>\d+)-(?P<end>\d+)(?::[+-])?$")


def parse_range(text: str) -> tuple:
    """A range literal -> ``(chrom, start, end)``, 0-based half-open.  The five formats of the reference's parser
    (src/giql/range_parser.py:78-89): ``chr1:1000-2000``, ``chr1:[1000,2000)``, ``chr1:[1001,2000]`` (closed: the
    end is made exclusive), ``chr1:1500`` (a point: ``[1500, 1501)``), and a trailing ``:+`` / ``:-`` on the first
    three -- the strand is read and dropped, the reference's predicate never looks at it.  No format matches: the
    reference's "Could not parse genomic range" ``ValueError``; ``start >= end`` as written: its ``ValueError``."""
    body = text.strip().strip("'\"")
    m = _POINT.match(body)
    if m:
        return m.group("chrom"), int(m.group("pos")), int(m.group("pos")) + 1
    m = _BRACKETED.match(body) or _DASHED.match(body)
    if not m:
        raise ValueError(f"Could not parse genomic range: '{text}'. Error: Invalid genomic range format: {body}")
    start, end = int(m.group("start")), int(m.group("end"))
    if start >= end:
        raise ValueError(f"Start must be less than end: {start} >= {end}")
    if m.groupdict().get("close") == "]":
        end += 1
    return m.group("chrom"), start, end


def _int64(v: int) -> int:
    """Saturated to int64.  The columns hold int32 (the kernel) or at most int64 (a residual): every comparison with
    a bound beyond that range has one outcome, and the saturated bound gives the same one."""
    return max(-(1 << 63), min((1 << 63) - 1, v))


#: op -> (comparison of ``start`` with its bound, comparison of ``end`` with its bound)
COMPARISONS = {"intersects": ("<", ">"), "contains": ("<=", ">="), "within": (">=", "<=")}


def bounds(op: str, rng: tuple, encoding: tuple) -> tuple:
    """``(bound on start, bound on end)`` of one canonical range for a table of ``encoding``: the literal the RAW
    ``start`` / ``end`` column is compared with (``COMPARISONS[op]``).  INTERSECTS compares ``start`` with the
    range's end and ``end`` with its start; CONTAINS (whose point form ``end > lo`` is ``end >= lo + 1`` on
    integers) and WITHIN compare like with like."""
    so, eo = CANONICAL_OFFSETS[tuple(encoding)]
    _chrom, lo, hi = rng
    if op == "intersects":
        return _int64(hi - so), _int64(lo - eo)
    return _int64(lo - so), _int64(hi - eo)


def make_set(op: str, quantifier: str, negated: bool, literals) -> RangeSet:
    """The set of a predicate as written: every literal parsed, duplicates dropped (an OR / AND does not count
    them), the order of first appearance kept."""
    ranges = []
    for text in literals:
        r = parse_range(text)
        if r not in ranges:
            ranges.append(r)
    return RangeSet(op, quantifier, bool(negated), tuple(ranges))


def needs_kernel(rs: RangeSet) -> bool:
    return rs.quantifier == "any" and len(rs.ranges) > 1


def fold(rs: RangeSet, side: PlanSide, group: int) -> list:
    """The residuals of a set that is a conjunction of comparisons: one range (a single literal, ANY / SOME over
    one), or ALL -- whose AND over the ranges is, exactly and also for NULLs, one ``chrom = c`` per distinct
    chromosome named, ``start`` against the tightest of its bounds and ``end`` against the tightest of its.  Negated,
    the conjunction is one OR-group (``group``) of the negated comparisons: De Morgan holds in three-valued logic."""
    from .shape import NEGATED_OP

    assert not needs_kernel(rs)
    start_op, end_op = COMPARISONS[rs.op]
    on_start, on_end = zip(*[bounds(rs.op, r, side.encoding) for r in rs.ranges])
    tight = {"<": min, "<=": min, ">": max, ">=": max}
    chroms = []
    for c, _lo, _hi in rs.ranges:
        if c not in chroms:
            chroms.append(c)
    terms = [(side.chrom_col, "=", Operand("str", c)) for c in chroms]
    terms.append((side.start_col, start_op, Operand("int", tight[start_op](on_start))))
    terms.append((side.end_col, end_op, Operand("int", tight[end_op](on_end))))
    if not rs.negated:
        return [Residual("where", Operand("l", col), op, rhs) for col, op, rhs in terms]
    return [Residual("where", Operand("l", col), NEGATED_OP[op], rhs, group) for col, op, rhs in terms]
