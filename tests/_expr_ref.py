"""A reference for computed SELECT-list columns (``HipEngine.eval_exprs`` / ``giql_hip_eval_expr_dev``), and a
seeded generator of expression sets for it.  No torch, no HIP library.

It wraps :func:`_sel_ref.values` -- the value-by-value statement of the expression semantics -- and adds what the
value path has on top of the filter:

* ``("if", cond, then, else)``: ``then`` where the Kleene value of ``cond`` is TRUE, ``else`` where it is FALSE or
  NULL (a searched CASE; both branches are evaluated, nothing can raise);
* ``("null",)``: an integer NULL (a CASE without ELSE);
* a NEGATIVE row id is the NULL row of its side: every column of that side reads as NULL, whatever its validity
  (the padded row of a LEFT join);
* the static type rule (:func:`can_float`): a float column or literal, the result of ``/``, arithmetic / NEG / ABS /
  LEAST / GREATEST over a float, ``if`` with a float branch -- such a tree has a float64 output, every other tree an
  int64 one; comparisons, IS [NOT] NULL, AND / OR / NOT and ``null`` are integers (TRUE / FALSE are 1 / 0);
* the final conversion: an integer value of a float64 output becomes ``float(int)`` (one round to nearest).

:class:`_sel_ref.Int64Overflow` is kept: an integer intermediate outside int64 is outside the contract.
"""
import math
import struct

import numpy as np

import _sel_ref
from _sel_ref import Int64Overflow  # noqa: F401  (re-exported: the callers catch it by this name)

LEAVES = ("a", "b", "lit")


# ---------------------------------------------------------------------------------------------- the reference
def _null_rows(spec, rows):
    """A column leaf's values with the NULL row (a negative id) read as None and nothing read through it."""
    safe = [r if r >= 0 else 0 for r in rows]
    if len(spec[1]) == 0:      # an empty table: every id is the NULL row
        return [None] * len(rows)
    vals = _sel_ref.values(spec, safe, safe)
    return [v if r >= 0 else None for v, r in zip(vals, rows)]


def values(tree, ra, rb):
    """The values of ``tree`` for the candidates ``(ra[i], rb[i])``: int / float / bool / None per candidate."""
    kind = tree[0]
    if kind == "expr":
        return values(tree[1], ra, rb)
    if kind == "a":
        return _null_rows(tree, ra)
    if kind == "b":
        return _null_rows(tree, rb)
    if kind == "lit":
        return _sel_ref.values(tree, ra, rb)
    if kind == "null":
        return [None] * len(ra)
    if kind == "if":
        cond, then, other = (values(c, ra, rb) for c in tree[1:])
        return [t if _sel_ref._truth(c) is True else e for c, t, e in zip(cond, then, other)]
    # every other node: evaluate the children here (they may hold if / null / NULL rows), then let _sel_ref apply
    # the operator to them as literal-free one-row columns would -- through its own per-value helpers
    args = [values(c, ra, rb) for c in tree[1:]]
    out = []
    for t in zip(*args):
        out.append(_apply(kind, t))
    return out


def _apply(kind, args):
    """One operator over already-computed values, by ``_sel_ref``'s own rules."""
    s = _sel_ref
    if kind in s.ARITH2:
        return s._arith(kind, args[0], args[1])
    if kind == "neg":
        x = args[0]
        return None if x is None else (-x if s._is_f(x) else s._fits(-_int(x)))
    if kind == "abs":
        x = args[0]
        return None if x is None else (abs(x) if s._is_f(x) else s._fits(abs(_int(x))))
    if kind in ("least", "greatest"):
        return s._extreme(kind == "least", args)
    if kind in s.CMP:
        x, y = args
        return None if x is None or y is None else s._cmp(kind, x, y)
    if kind == "isnull":
        return args[0] is None
    if kind == "notnull":
        return args[0] is not None
    if kind == "not":
        return None if args[0] is None else not s._truth(args[0])
    if kind == "and":
        return s._and(args)
    if kind == "or":
        return s._or(args)
    raise ValueError(f"node kind {kind!r}")


def _int(v):
    return int(v) if isinstance(v, (bool, np.bool_)) else v


def can_float(tree) -> bool:
    """The static type rule: can the tree's value be a float?"""
    kind = tree[0]
    if kind == "expr":
        return can_float(tree[1])
    if kind == "lit":
        return isinstance(tree[1], float) or (isinstance(tree[1], np.floating))
    if kind in ("a", "b"):
        return tree[1].dtype.kind == "f"
    if kind == "/":
        return True
    if kind == "if":
        return can_float(tree[2]) or can_float(tree[3])
    if kind in ("+", "-", "*", "neg", "abs", "least", "greatest"):
        return any(can_float(c) for c in tree[1:])
    return False


def evaluate(tree, ia=None, ib=None, n=None):
    """What ``HipEngine.eval_exprs([tree], ia, ib, n)`` returns for the tree, on the host: ``(values, valid)`` --
    ``values`` a float64 or int64 numpy array by the static type rule (0 where NULL), ``valid`` a uint8 array."""
    if n is None:
        n = len(ia if ia is not None else ib)
    ra = list(range(n)) if ia is None else [int(x) for x in ia]
    rb = list(range(n)) if ib is None else [int(x) for x in ib]
    vals = values(tree, ra, rb)
    fl = can_float(tree)
    out = np.zeros(n, np.float64 if fl else np.int64)
    valid = np.ones(n, np.uint8)
    for i, v in enumerate(vals):
        if v is None:
            valid[i] = 0
        elif fl:
            out[i] = float(_int(v))            # the final conversion: one round to nearest for an integer
        else:
            assert not isinstance(v, float), "the static type rule called a float value an integer"
            out[i] = _sel_ref._fits(_int(v))
    return out, valid


def bits(x) -> np.ndarray:
    """A float64 array as its bit patterns, every NaN as one pattern (a NaN's payload is not specified)."""
    x = np.ascontiguousarray(x, np.float64)
    b = x.view(np.uint64).copy()
    b[np.isnan(x)] = struct.unpack("<Q", struct.pack("<d", math.nan))[0]
    return b


def count_nodes(tree) -> int:
    """The postfix nodes ``HipEngine._flatten_expr`` makes of a tree."""
    if tree[0] == "expr":
        return count_nodes(tree[1])
    if tree[0] == "null":
        return 1
    if tree[0] == "if":
        return 1 + sum(count_nodes(c) for c in tree[1:])
    if tree[0] in LEAVES:
        return 1
    kids = sum(count_nodes(c) for c in tree[1:])
    return kids + (1 if tree[0] in _sel_ref.UNARY or tree[0] not in _sel_ref.NARY else len(tree) - 2)


def live_values(tree) -> int:
    """The most values the postfix form keeps live at once (``if``: cond, then, else stay until the node)."""
    if tree[0] == "expr":
        return live_values(tree[1])
    if tree[0] in LEAVES or tree[0] == "null":
        return 1
    return max(live_values(c) + k for k, c in enumerate(tree[1:])) if tree[0] == "if" else \
        max(live_values(c) + (1 if k else 0) for k, c in enumerate(tree[1:]))


def node_kinds(tree, out=None) -> set:
    out = set() if out is None else out
    if tree[0] == "expr":
        return node_kinds(tree[1], out)
    if tree[0] in LEAVES:
        return out
    out.add(tree[0])
    for c in tree[1:]:
        node_kinds(c, out)
    return out


# ---------------------------------------------------------------------------------------------- the generator
class ExprDraw(_sel_ref.Draw):
    """One generated ``eval_exprs`` call: the columns of ``_sel_ref.Draw`` and ``n_trees`` expression trees built with
    its ``_arith`` / ``_bool`` / ``_deep_arith`` (which prove integer bounds), wrapped in ``if`` / ``null`` nodes.
    The first tree is a deep one (the depth rotates with the seed), the second is filled up to 256 nodes on one
    seed in three; the candidates hold padded (-1) ids on side B, side A and both."""

    def __init__(self, seed, attempt=0, n_trees=8):
        self.n_trees = n_trees
        self.trees = []
        super().__init__(seed, attempt)

    def _wrap(self, x):
        """``x`` under a searched CASE: ``if(cond, x, other | null)`` or ``if(cond, other, x)``."""
        rng = self.rng
        cond = self._bool(rng.choice((2, 3, 4)))
        r = rng.random()
        if r < 0.35:
            return ("if", cond, x, ("null",))
        other = self._arith(rng.choice((1, 2))).tree
        return ("if", cond, x, other) if r < 0.7 else ("if", cond, other, x)

    def _build(self):
        rng = self.rng
        depth = 1 + self.seed % _sel_ref.MAX_LIVE
        trees = [self._deep_arith(depth).tree]
        if self.seed % 3 == 0:
            trees.append(self._padding(_sel_ref.MAX_NODES)[1])
        while len(trees) < self.n_trees:
            r = rng.random()
            size = rng.choice((1, 2, 3, 4, 6, 9))
            if r < 0.45:
                t = self._wrap(self._arith(size).tree)
            elif r < 0.55:
                t = self._wrap(self._wrap(self._arith(size).tree))       # a CASE inside a CASE
            elif r < 0.7:
                t = ("+", self._wrap(("lit", rng.randint(-3, 3))), ("lit", 1))   # a CASE inside arithmetic
            elif r < 0.85:
                t = self._arith(size).tree
            else:
                t = self._bool(2 * size)                                 # a condition as a value: 0 / 1 / NULL
            if live_values(t) <= _sel_ref.MAX_LIVE and count_nodes(t) <= _sel_ref.MAX_NODES:
                trees.append(t)
        self.trees = trees
        self.depths.add(("expr", max(live_values(t) for t in trees)))
        self.depths.add(("expr-first", live_values(trees[0])))

    def _population_mask(self):
        return [True, False]        # (no predicates here: the keep share of _sel_ref.draw has no meaning)

    def candidates(self, n):
        """``n`` candidate pairs; about one in eight has a -1 on side B, one in eight on side A, some on both."""
        rng = np.random.default_rng(self.seed * 31 + n)
        ia = rng.integers(0, self.N_A, n).astype(np.int32)
        ib = rng.integers(0, self.N_B, n).astype(np.int32)
        pad = rng.integers(0, 8, n)
        ib[(pad == 0) | (pad == 2)] = -1
        ia[(pad == 1) | (pad == 2)] = -1
        return ia, ib

    def expected(self, ia, ib):
        """``[(values, valid)]`` per tree; each distinct ``(ia, ib)`` is evaluated once.  Raises Int64Overflow."""
        n = len(ia)
        if n == 0:
            return [evaluate(t, [], []) for t in self.trees]
        uniq, inverse = np.unique(np.stack([np.asarray(ia, np.int64), np.asarray(ib, np.int64)], 1), axis=0,
                                  return_inverse=True)
        inverse = np.asarray(inverse).reshape(-1)
        out = []
        for t in self.trees:
            v, ok = evaluate(t, uniq[:, 0], uniq[:, 1])
            out.append((v[inverse], ok[inverse]))
        return out


MAX_ATTEMPTS = _sel_ref.MAX_ATTEMPTS


def draw(seed, n, n_trees=8):
    """The draw of ``seed`` for ``n`` candidates and what the reference gives for it: ``(draw, ia, ib, expected)``.
    Re-drawn (at most ``MAX_ATTEMPTS`` times, as ``_sel_ref.draw``) while the reference overflows int64 -- while
    building the trees or on the candidates and the whole population."""
    for attempt in range(MAX_ATTEMPTS):
        try:
            d = ExprDraw(seed, attempt, n_trees)
            ia, ib = d.candidates(n)
            expected = d.expected(ia, ib)
            # the population with and without NULL rows: a re-draw must not depend on n
            d.expected(np.array(d.pa + [-1, 0, -1]), np.array(d.pb + [0, -1, -1]))
        except Int64Overflow:
            continue
        d.attempt = attempt
        return d, ia, ib, expected
    raise AssertionError(f"seed {seed}: the reference overflows int64 in all {MAX_ATTEMPTS} attempts")


#: the seeds and candidate counts of the GPU differential test (tests/test_select_expressions_gpu.py)
SIZES = _sel_ref.SIZES
BIG = _sel_ref.BIG
GPU_CASES = [(seed, n) for seed, n in enumerate(SIZES)] + [(seed, BIG) for seed in range(len(SIZES), 14)]
