"""A reference for the residual expression evaluator, and a seeded generator of predicate sets for it.

No torch, no HIP library: numpy arrays stand where ``HipEngine.select`` takes tensors.

The reference (:func:`evaluate`) is written from the documented semantics (the comments of
``select_kernels.hip.h`` on arithmetic operands and on the conjunction of clauses, DESIGN section 4b "Residual
predicates"), on plain Python values: ``int`` is exact and unbounded, ``float`` is binary64, ``None`` is NULL,
``True`` / ``False`` / ``None`` are Kleene values.

* integer ``+ - * neg abs`` stay integers; any float argument makes the operation binary64, the integer converted
  with ``float(int)`` (round to nearest even);
* ``/`` is always a binary64 division of the two converted arguments, NULL on a zero divisor (``-0.0`` included);
* NULL propagates through arithmetic and comparisons; a mixed comparison converts its integer the same way;
* LEAST / GREATEST skip NULL arguments and give NULL only when all are NULL;
* AND / OR / NOT are Kleene's; IS [NOT] NULL is never NULL;
* a predicate keeps a candidate only when TRUE; neighbours sharing a non-zero group are OR-ed, clauses AND-ed;
* float32 columns widen exactly, uint8 reads 0..255.

NaN is unspecified upstream (the reference project's two engines disagree) and IEEE here: every comparison with a
NaN is false except ``!=``, LEAST / GREATEST fold their arguments left to right with ``<`` / ``>`` (so a NaN stays
only where it is the first non-NULL argument), and a NaN is not zero, hence TRUE under IS TRUE / AND / OR / NOT.

Every integer intermediate must fit int64: the reference raises :class:`Int64Overflow` (an error in the execution
target the semantics come from, a wrap in the kernel; out of scope).

Types are dynamic, as in the kernel: LEAST / GREATEST over an integer and a float argument is a float where both
are present and keeps the integer where the float is NULL.  With a NULL beside it the kernel therefore keeps an
integer past 2^53 exact where a statically typed engine would have rounded it to a double; the generator does not
produce that (integers beside floats under LEAST / GREATEST stay within +-2^53, where the cast is exact).
"""
import math
import random

import numpy as np

I64_MIN, I64_MAX = -(2**63), 2**63 - 1
CMP = ("=", "!=", "<", "<=", ">", ">=")
ARITH2 = ("+", "-", "*", "/")
UNARY = ("neg", "abs", "isnull", "notnull", "not")
NARY = ("least", "greatest", "and", "or")
KINDS = ARITH2 + ("neg", "abs", "least", "greatest") + CMP + ("isnull", "notnull", "and", "or", "not")
MAX_NODES, MAX_LIVE, MAX_PREDS = 256, 12, 16


class Int64Overflow(ArithmeticError):
    pass


# ---------------------------------------------------------------------------------------------- the reference
def _fits(v):
    if not I64_MIN <= v <= I64_MAX:
        raise Int64Overflow(v)
    return v


def _is_f(v):
    return isinstance(v, float)


def _cmp(op, a, b):
    """One comparison of two non-NULL numbers: exact between integers, binary64 as soon as one is a float."""
    if _is_f(a) or _is_f(b):
        a, b = float(a), float(b)
    if op == "=":
        return a == b
    if op == "!=":
        return a != b
    if op == "<":
        return a < b
    if op == "<=":
        return a <= b
    if op == ">":
        return a > b
    return a >= b


def _arith(op, a, b):
    if a is None or b is None:
        return None
    if op == "/":
        a, b = float(a), float(b)
        return None if b == 0.0 else a / b
    if _is_f(a) or _is_f(b):
        a, b = float(a), float(b)
        return a + b if op == "+" else (a - b if op == "-" else a * b)
    return _fits(a + b if op == "+" else (a - b if op == "-" else a * b))


def _extreme(least, args):
    out = None
    for v in args:
        if v is None:
            continue
        if out is None:
            out = v
        elif _is_f(out) or _is_f(v):
            x, y = float(out), float(v)
            out = (y if y < x else x) if least else (y if y > x else x)
        else:
            out = min(out, v) if least else max(out, v)
    return out


def _truth(v):
    """A value as a Kleene value: NULL stays NULL, a number is TRUE unless it is zero."""
    return None if v is None else bool(v != 0)


def _and(args):
    ts = [_truth(a) for a in args]
    return False if any(t is False for t in ts) else (None if any(t is None for t in ts) else True)


def _or(args):
    ts = [_truth(a) for a in args]
    return True if any(t is True for t in ts) else (None if any(t is None for t in ts) else False)


def _column_values(spec, rows):
    col = spec[1]
    valid = spec[2] if len(spec) > 2 else None
    if col.dtype.kind == "f":
        vals = [float(col[r]) for r in rows]          # float32 widens exactly
    else:
        vals = [int(col[r]) for r in rows]            # bool / uint8 read 0..255
    if valid is not None:
        vals = [v if valid[r] else None for v, r in zip(vals, rows)]
    return vals


def _literal(v):
    if isinstance(v, (bool, np.bool_)):
        return int(v)
    if isinstance(v, (int, np.integer)):
        return _fits(int(v))
    return float(v)


def values(spec, ra, rb):
    """The values of one operand -- ``("a" | "b", column[, valid])``, ``("lit", v)``, ``("expr", tree)`` or a tree --
    for the candidates whose row ids are the lists ``ra`` / ``rb``: a list of int / float / bool / None."""
    kind = spec[0]
    if kind == "expr":
        return values(spec[1], ra, rb)
    if kind == "lit":
        return [_literal(spec[1])] * len(ra)
    if kind == "a":
        return _column_values(spec, ra)
    if kind == "b":
        return _column_values(spec, rb)
    args = [values(c, ra, rb) for c in spec[1:]]
    if kind in ARITH2:
        return [_arith(kind, x, y) for x, y in zip(*args)]
    if kind == "neg":
        return [None if x is None else (-x if _is_f(x) else _fits(-x)) for x in args[0]]
    if kind == "abs":
        return [None if x is None else (abs(x) if _is_f(x) else _fits(abs(x))) for x in args[0]]
    if kind in ("least", "greatest"):
        return [_extreme(kind == "least", t) for t in zip(*args)]
    if kind in CMP:
        return [None if x is None or y is None else _cmp(kind, x, y) for x, y in zip(*args)]
    if kind == "isnull":
        return [x is None for x in args[0]]
    if kind == "notnull":
        return [x is not None for x in args[0]]
    if kind == "not":
        return [None if x is None else not _truth(x) for x in args[0]]
    if kind == "and":
        return [_and(t) for t in zip(*args)]
    if kind == "or":
        return [_or(t) for t in zip(*args)]
    raise ValueError(f"node kind {kind!r}")


def holds(op, xs, ys=None):
    """One predicate over operand values: TRUE or not (a filter does not tell FALSE from NULL)."""
    if op == "istrue":
        return [_truth(x) is True for x in xs]
    if op == "isnull":
        return [x is None for x in xs]
    if op == "notnull":
        return [x is not None for x in xs]
    op = {"==": "=", "<>": "!="}.get(op, op)
    return [x is not None and y is not None and _cmp(op, x, y) for x, y in zip(xs, ys)]


def clauses(preds):
    """Predicates are AND-ed; neighbours sharing a non-zero group are one OR clause."""
    out, prev = [], 0
    for p in preds:
        g = p[3] if len(p) > 3 else 0
        if out and g != 0 and g == prev:
            out[-1].append(p)
        else:
            out.append([p])
        prev = g
    return out


def evaluate(preds, ia=None, ib=None, n=None):
    """The keep mask of ``HipEngine.select(preds, idx_a=ia, idx_b=ib, n=n)``: one bool per candidate.  A missing id
    array means "the candidate index".  Each distinct ``(ia, ib)`` is evaluated once."""
    if n is None:
        n = len(ia if ia is not None else ib)
    ia = np.arange(n, dtype=np.int64) if ia is None else np.asarray(ia, np.int64)
    ib = np.arange(n, dtype=np.int64) if ib is None else np.asarray(ib, np.int64)
    if n == 0:
        return np.zeros(0, bool)
    uniq, inverse = np.unique(np.stack([ia, ib], 1), axis=0, return_inverse=True)
    ra, rb = uniq[:, 0].tolist(), uniq[:, 1].tolist()
    keep = [True] * len(ra)
    for clause in clauses(preds):
        acc = [False] * len(ra)
        for p in clause:
            xs = values(p[0], ra, rb)
            t = holds(p[1], xs, values(p[2], ra, rb) if p[1] not in ("isnull", "notnull", "istrue") else None)
            acc = [u or v for u, v in zip(acc, t)]
        keep = [u and v for u, v in zip(keep, acc)]
    return np.asarray(keep, bool)[np.asarray(inverse).reshape(-1)]


def count_nodes(tree) -> int:
    """The nodes ``HipEngine._flatten_expr`` makes of a tree (an n-ary node of k arguments is k - 1 binary ones)."""
    if tree[0] == "expr":
        return count_nodes(tree[1])
    if tree[0] in ("a", "b", "lit"):
        return 1
    kids = sum(count_nodes(c) for c in tree[1:])
    return kids + (1 if tree[0] in UNARY or tree[0] not in NARY else len(tree) - 2)


def live_values(tree) -> int:
    """The most values the postfix form keeps live at once."""
    if tree[0] == "expr":
        return live_values(tree[1])
    if tree[0] in ("a", "b", "lit"):
        return 1
    return max(live_values(c) + (1 if k else 0) for k, c in enumerate(tree[1:]))


def pred_nodes(preds) -> int:
    return sum(count_nodes(o) for p in preds for o in (p[0], p[2]) if o[0] == "expr")


# ---------------------------------------------------------------------------------------------- value pools
F32_TENTH = float(np.float32(0.1))
# 0, +-1, INT32_MIN / MAX (-2^31 is INT32_MIN), 2^31, 2^53 and its neighbours, the ends of int64
INT_EDGES = (0, 1, -1, -(2**31), 2**31 - 1, 2**31, 2**53, 2**53 + 1, 2**53 - 1, I64_MAX, I64_MIN + 1, I64_MIN)
FLOAT_EDGES = (0.0, -0.0, 5e-324, F32_TENTH, 2.0**53, 2.0**63, 1e308, math.inf, -math.inf, math.nan)
TYPES = ("i32", "i64", "f32", "f64", "u8")
_DT = {"i32": np.int32, "i64": np.int64, "f32": np.float32, "f64": np.float64, "u8": np.uint8}


def edge_key(v):
    """A hashable name for an edge value that tells -0.0 from 0.0, a float from an integer, and finds NaN."""
    if isinstance(v, float):
        return ("f", "nan") if math.isnan(v) else ("f", math.copysign(1.0, v), abs(v))
    return ("i", int(v))


ALL_EDGES = frozenset(edge_key(v) for v in INT_EDGES + FLOAT_EDGES)


class Column:
    """A generated column: ``bound`` is the largest |value| of an integer column (None for a float one) -- the
    generator adds and multiplies integers only where the bounds prove that int64 holds the result; ``cmp_only``
    marks the column that holds INT64_MIN."""

    def __init__(self, side, name, typ, data, valid, bound, cmp_only=False):
        self.side, self.name, self.typ, self.data, self.valid = side, name, typ, data, valid
        self.bound, self.cmp_only = bound, cmp_only
        self.nullness = "none" if valid is None else ("all" if not valid.any() else "some")

    @property
    def spec(self):
        return (self.side, self.data) if self.valid is None else (self.side, self.data, self.valid)

    def edges(self):
        ok = np.ones(len(self.data), bool) if self.valid is None else self.valid.astype(bool)
        conv = float if self.data.dtype.kind == "f" else int
        return {edge_key(conv(v)) for v in self.data[ok]} & ALL_EDGES


def _fill(rng, n, edges, draw, dtype):
    vals = list(edges) + [draw() for _ in range(n - len(edges))]
    rng.shuffle(vals)
    return np.array(vals[:n], dtype=dtype)


def make_columns(rng, side, n):
    """The columns of one side: every operand type, tame and edge-laden, each with or without a validity mask
    (drawn), and one all-NULL column."""
    ri = rng.randint
    big32 = lambda: rng.choice((-1, 1)) * ri(1518500250, 2**31 - 1)     # |v| in [2^30.5, 2^31): products reach 2^62
    f_edges32 = (0.0, -0.0, float(np.float32(2.0**-149)), F32_TENTH, 2.0**53, 2.0**63, math.inf, -math.inf, math.nan)
    mid = (0, 1, -1, -(2**31), 2**31 - 1, 2**31, 2**53, 2**53 + 1, 2**53 - 1, -(2**53), -(2**53) - 1)
    table = [
        # name, type, edges, draw, bound, cmp_only
        ("i32_small", "i32", (0, 1, -1), lambda: ri(-6, 6), 6, False),
        ("i32_edge", "i32", (0, 1, -1, -(2**31), 2**31 - 1), lambda: ri(-(2**31), 2**31 - 1), 2**31, False),
        ("i32_big", "i32", (), big32, 2**31, False),
        ("i64_small", "i64", (0, 1, -1), lambda: ri(-1000, 1000), 1000, False),
        ("i64_mid", "i64", mid, lambda: ri(-(2**53), 2**53), 2**53 + 1, False),
        ("i64_huge", "i64", mid + (I64_MAX, I64_MIN + 1, I64_MAX - 1), lambda: ri(I64_MIN + 1, I64_MAX), I64_MAX, False),
        ("i64_min", "i64", (I64_MIN, I64_MIN + 1, I64_MAX, 0, -1), lambda: ri(I64_MIN, I64_MAX), 2**63, True),
        ("f32_tame", "f32", (0.0, F32_TENTH), lambda: rng.gauss(0, 3), None, False),
        ("f32_edge", "f32", f_edges32, lambda: rng.gauss(0, 1e6), None, False),
        ("f64_tame", "f64", (0.0, 0.5), lambda: rng.gauss(0, 3), None, False),
        ("f64_edge", "f64", FLOAT_EDGES, lambda: rng.gauss(0, 1e6), None, False),
        ("f64_int", "f64", (2.0**53, 2.0**63, -(2.0**63), 2.0**31), lambda: float(ri(-(2**53), 2**53)), None, False),
        ("u8", "u8", (0, 1, 255), lambda: ri(0, 255), 255, False),
        ("u8_bit", "u8", (0, 1), lambda: ri(0, 1), 1, False),
    ]
    cols = []
    for name, typ, edges, draw, bound, cmp_only in table:
        data = _fill(rng, n, edges, draw, _DT[typ])
        valid = None
        if rng.random() < 0.5:
            valid = np.array([rng.random() > 0.25 for _ in range(n)], np.uint8)
        cols.append(Column(side, name, typ, data, valid, bound, cmp_only))
    typ = rng.choice(TYPES)
    data = _fill(rng, n, (), {"i32": lambda: ri(-9, 9), "i64": lambda: ri(-9, 9), "u8": lambda: ri(0, 9),
                              "f32": lambda: rng.gauss(0, 1), "f64": lambda: rng.gauss(0, 1)}[typ], _DT[typ])
    cols.append(Column(side, "all_null", typ, data, np.zeros(n, np.uint8), None if typ[0] == "f" else 9))
    return cols


# ---------------------------------------------------------------------------------------------- the generator
class _X:
    """A generated expression: its tree and what the generator knows of it -- ``bound`` (the largest |value| it can
    take as an integer; None when it is a float whatever the NULLs) -- and ``floaty`` (it may be a float)."""

    def __init__(self, tree, bound, floaty):
        self.tree, self.bound, self.floaty = tree, bound, floaty


LIT_INTS = (0, 1, -1, 2, 3, 7, -(2**31), 2**31 - 1, 2**31, 2**53, 2**53 + 1, 2**53 - 1, I64_MAX, I64_MIN + 1)
LIT_FLOATS = (0.0, -0.0, 0.5, 1.5, -2.25, 5e-324, F32_TENTH, 2.0**53, 2.0**63, 1e308, math.inf, -math.inf, math.nan)


class Draw:
    """One generated call: the columns of both sides, the predicates, and what they cover."""

    N_A, N_B = 61, 53

    def __init__(self, seed, attempt=0, plain_only=False):
        self.seed, self.attempt, self.plain_only = seed, attempt, plain_only
        self.rng = rng = random.Random(seed * 1000 + attempt)
        self.cols = {"a": make_columns(rng, "a", self.N_A), "b": make_columns(rng, "b", self.N_B)}
        # the population every candidate is drawn from: all row pairs
        self.pa = [i for i in range(self.N_A) for _ in range(self.N_B)]
        self.pb = [j for _ in range(self.N_A) for j in range(self.N_B)]
        self.kinds, self.depths, self.cmp_pairs, self.arith_pairs = set(), set(), set(), set()
        self.edges, self.nullness, self.lit_kinds, self.arities, self.pred_forms = set(), set(), set(), set(), set()
        self.rot = seed * 7                       # rotates through the 25 ordered type pairs
        self.preds, self.budget = [], MAX_NODES
        self._build()
        self.n_nodes = pred_nodes(self.preds)
        self.mask = self._population_mask()
        self.share = sum(self.mask) / len(self.mask)

    # ---- leaves
    def _col(self, typ=None, max_bound=None, side=None, allow_cmp_only=False):
        pool = [c for s in ("a", "b") if side in (None, s) for c in self.cols[s]
                if (typ is None or c.typ == typ) and (allow_cmp_only or not c.cmp_only)
                and (max_bound is None or c.bound is None or c.bound <= max_bound)]
        c = self.rng.choice(pool)
        self.edges |= c.edges()
        self.nullness.add(c.nullness)
        return c

    def _leaf_col(self, **kw):
        c = self._col(**kw)
        return _X(c.spec, c.bound, c.bound is None), c.typ

    def _lit(self, floaty=None, max_bound=None):
        rng = self.rng
        if floaty is None:
            floaty = rng.random() < 0.5
        if floaty:
            v = rng.choice(LIT_FLOATS) if rng.random() < 0.7 else rng.gauss(0, 10)
            self.lit_kinds.add("float")
            self.edges |= {edge_key(v)} & ALL_EDGES
            return _X(("lit", v), None, True)
        pool = [v for v in LIT_INTS if max_bound is None or abs(v) <= max_bound]
        v = rng.choice(pool) if rng.random() < 0.7 else rng.randint(-9, 9)
        self.lit_kinds.add("int")
        self.edges |= {edge_key(v)} & ALL_EDGES
        return _X(("lit", v), abs(v), False)

    def _leaf(self, max_bound=None):
        if self.rng.random() < 0.2:
            return self._lit(max_bound=max_bound)
        return self._leaf_col(max_bound=max_bound)[0]

    def _next_pair(self):
        self.rot += 1
        return TYPES[self.rot % 5], TYPES[(self.rot // 5) % 5]

    # ---- arithmetic
    def _combine(self, op, x, y):
        """``x op y`` when int64 provably holds every integer result, else None."""
        self.kinds.add(op)
        tree = (op, x.tree, y.tree)
        if op == "/":
            return _X(tree, None, True)
        if x.bound is None or y.bound is None:
            return _X(tree, None, True)
        b = x.bound * y.bound if op == "*" else x.bound + y.bound
        if b > I64_MAX:
            return None
        return _X(tree, b, x.floaty or y.floaty)

    def _typed_pair(self, sink, max_bound=2**53 + 1):
        """Two column leaves of the next ordered type pair, recorded in ``sink``."""
        tx, ty = self._next_pair()
        sink.add((tx, ty))
        return self._leaf_col(typ=tx, max_bound=max_bound)[0], self._leaf_col(typ=ty, max_bound=2**31)[0]

    def _arith(self, size):
        """An arithmetic expression of about ``size`` leaves."""
        rng = self.rng
        if size <= 1:
            x = self._leaf()
            if rng.random() < 0.25 and (x.bound is None or x.bound <= I64_MAX):
                op = rng.choice(("neg", "abs"))
                self.kinds.add(op)
                x = _X((op, x.tree), x.bound, x.floaty)
            return x
        if size == 2 and rng.random() < 0.6:
            x, y = self._typed_pair(self.arith_pairs)
            for op in rng.sample(ARITH2, 4):
                z = self._combine(op, x, y)
                if z is not None:
                    return z
        if rng.random() < 0.3:
            return self._extreme(size)
        left = rng.randint(1, size - 1)
        x, y = self._arith(left), self._arith(size - left)
        for op in rng.sample(ARITH2, 4):
            z = self._combine(op, x, y)
            if z is not None:
                return z
        raise AssertionError("a division always combines")

    def _extreme(self, size):
        """LEAST / GREATEST of 1..4 arguments; integers beside floats stay within +-2^53 (leaves only)."""
        rng = self.rng
        op = rng.choice(("least", "greatest"))
        k = rng.randint(1, 4)
        self.kinds.add(op)
        self.arities.add((op, k))
        mixed = rng.random() < 0.5
        if mixed:
            args = [self._leaf(max_bound=2**53) for _ in range(k)]
            if k == 2 and rng.random() < 0.5:
                args = list(self._typed_pair(self.arith_pairs, max_bound=2**53))
        else:
            floaty = rng.random() < 0.5
            args = []
            for _ in range(k):
                if floaty:
                    args.append(self._lit(floaty=True) if rng.random() < 0.2 else
                                self._leaf_col(typ=rng.choice(("f32", "f64")))[0])
                else:
                    sub = max(1, size // k)
                    x = self._arith(sub) if sub > 1 and rng.random() < 0.4 else None
                    if x is None or x.bound is None or x.floaty:
                        x = self._lit(floaty=False) if rng.random() < 0.2 else self._leaf_col(typ=rng.choice(("i32", "i64", "u8")))[0]
                    args.append(x)
        bounds = [a.bound for a in args]
        bound = None if all(b is None for b in bounds) else max(b for b in bounds if b is not None)
        return _X((op, *[a.tree for a in args]), bound, any(a.floaty for a in args))

    def _deep_arith(self, live):
        """A right-nested tree that keeps exactly ``live`` values: x1 op (x2 op (... op x_live))."""
        rng = self.rng
        x = self._leaf(max_bound=2**31)
        for _ in range(live - 1):
            y = self._leaf(max_bound=2**31)
            z = None
            for op in rng.sample(("+", "-", "*", "/", "least"), 5):
                if op == "least":
                    if (y.bound is None) == (x.bound is None):
                        self.kinds.add("least")
                        z = _X(("least", y.tree, x.tree), x.bound and max(x.bound, y.bound), x.floaty or y.floaty)
                else:
                    z = self._combine(op, y, x)
                if z is not None:
                    break
            x = z
        assert live_values(x.tree) == live
        self.depths.add(("arith", live))
        return x

    # ---- booleans
    def _comparison(self, size):
        rng = self.rng
        op = rng.choice(CMP)
        self.kinds.add(op)
        r = rng.random()
        if size <= 2 and r < 0.5:
            x, y = self._typed_pair(self.cmp_pairs)
        elif size <= 2 and r < 0.65:
            x, y = self._leaf_col(typ="i64", allow_cmp_only=True)[0], self._leaf_col(allow_cmp_only=True)[0]
        elif size <= 2:
            x, y = self._leaf(), self._leaf()
        else:
            left = rng.randint(1, size - 1)
            x, y = self._arith(left), self._arith(size - left)
        return (op, x.tree, y.tree)

    def _bool(self, size):
        rng = self.rng
        r = rng.random()
        if size <= 2:
            if r < 0.2:
                op = rng.choice(("isnull", "notnull"))
                self.kinds.add(op)
                return (op, self._arith(size).tree)
            return self._comparison(size)
        if r < 0.15:
            self.kinds.add("not")
            return ("not", self._bool(size - 1))
        if r < 0.25:
            op = rng.choice(("isnull", "notnull"))
            self.kinds.add(op)
            return (op, self._arith(size).tree)
        if r < 0.4:
            return self._comparison(size)
        op = rng.choice(("and", "or"))
        k = rng.randint(1, 4)
        self.kinds.add(op)
        self.arities.add((op, k))
        return (op, *[self._bool(max(2, size // k)) for _ in range(k)])

    def _deep_bool(self, live):
        """A right-nested boolean tree that keeps exactly ``live`` values: every level holds one IS [NOT] NULL
        result while the rest is evaluated; the innermost term is a comparison of two leaves (two values)."""
        rng = self.rng

        def null_test():
            op = rng.choice(("isnull", "notnull"))
            self.kinds.add(op)
            return (op, self._leaf_col()[0].tree)

        if live == 1:
            tree = null_test()
        else:
            tree = self._comparison(2)
            for _ in range(live - 2):
                op = rng.choice(("and", "or"))
                self.kinds.add(op)
                tree = (op, null_test(), tree)
        assert live_values(tree) == live
        self.depths.add(("bool", live))
        return tree

    # ---- predicates
    def _operand(self, size):
        """One side of a plain comparison: a program of about ``size`` leaves, or a plain column / literal."""
        if self.plain_only or size <= 1 and self.rng.random() < 0.7:
            return self._leaf().tree if self.rng.random() < 0.8 else self._leaf_col(allow_cmp_only=True)[0].tree
        return ("expr", self._arith(size).tree)

    def _candidate(self, k):
        """The k-th predicate before its operator is chosen: (form, lhs, rhs)."""
        rng = self.rng
        left = self.budget - pred_nodes(self.preds)
        size = max(1, min(rng.choice((1, 2, 2, 3, 4, 6, 9)), left // 6))
        if self.plain_only or left < 8:
            if rng.random() < 0.25:
                return "null", self._leaf_col()[0].tree, ("lit", 0)
            if rng.random() < 0.6:
                x, y = self._typed_pair(self.cmp_pairs)
                return "cmp", x.tree, y.tree
            return "cmp", self._leaf_col(allow_cmp_only=True)[0].tree, self._leaf().tree
        # the two deep programs of this draw come first: the depth rotates with the seed
        if k == 0:
            return "cmp", ("expr", self._deep_arith(1 + self.seed % MAX_LIVE).tree), self._leaf().tree
        if k == 1:
            return "true", ("expr", self._deep_bool(1 + (self.seed * 5 + 3) % MAX_LIVE)), ("lit", 0)
        r = rng.random()
        if r < 0.3:
            return "true", ("expr", self._bool(2 * size)), ("lit", 0)
        if r < 0.4:
            return "null", ("expr", self._arith(size + 1).tree), ("lit", 0)
        if r < 0.45:
            return "true", ("expr", self._arith(size + 1).tree), ("lit", 0)    # a number IS TRUE unless it is zero
        if r < 0.55:
            return "null", self._leaf_col()[0].tree, ("lit", 0)
        if r < 0.7:
            x, y = self._typed_pair(self.cmp_pairs)
            return "cmp", x.tree, y.tree
        return "cmp", self._operand(size), self._operand(rng.choice((1, size)))

    def _choices(self, form, lhs, rhs):
        """Every predicate the candidate can become, with its TRUE mask over the population."""
        xs = values(lhs, self.pa, self.pb)
        if form == "cmp":
            ys = values(rhs, self.pa, self.pb)
            return [((lhs, op, rhs), holds(op, xs, ys)) for op in CMP]
        if form == "null":
            return [((lhs, op, rhs), holds(op, xs)) for op in ("isnull", "notnull")]
        out = [((lhs, "istrue", rhs), holds("istrue", xs))]
        if lhs[0] == "expr" and count_nodes(lhs) < 200:
            neg = ("expr", ("not", lhs[1]))
            self.kinds.add("not")
            out.append(((neg, "istrue", rhs), holds("istrue", values(neg, self.pa, self.pb))))
        return out

    def _build(self):
        """Predicates one by one; the operator of each is drawn among those that leave at least 4 % -- and most of
        what was left -- of the population; a predicate with no such operator joins its predecessor's OR group
        (which can only keep more).  One draw in three is filled up to exactly 256 nodes."""
        rng = self.rng
        full = not self.plain_only and self.seed % 3 == 0
        n_preds = rng.randint(1, 4) if self.seed % 4 == 1 else rng.randint(6, MAX_PREDS)
        if full:
            n_preds, self.budget = MAX_PREDS, MAX_NODES - 9
        total = len(self.pa)
        done, last = [True] * total, None          # the AND of the closed clauses; the open clause's OR
        group = 0
        for k in range(n_preds):
            if full and k == n_preds - 1:
                form, lhs, rhs = "cmp", self._padding(MAX_NODES - pred_nodes(self.preds)), ("lit", 0)
            else:
                form, lhs, rhs = self._candidate(k)
            options = self._choices(form, lhs, rhs)
            cur = [u and v for u, v in zip(done, last)] if last is not None else done
            have = sum(cur)
            scored = [(p, m, sum(u and v for u, v in zip(cur, m))) for p, m in options]
            good = [s for s in scored if s[2] >= max(0.04 * total, 0.7 * have)]
            if have == total and any(s[2] <= 0.9 * total for s in good):      # nothing dropped yet: drop something
                good = [s for s in good if s[2] <= 0.9 * total]
            join = last is not None and (not good or rng.random() < 0.25)
            if join:                                            # OR into the open clause
                p, m, _ = rng.choice(scored)
                if self.preds[-1][3] == 0:
                    group += 1
                    self.preds[-1] = self.preds[-1][:3] + (group,)
                last = [u or v for u, v in zip(last, m)]
                self.preds.append(p + (self.preds[-1][3],))
                self.pred_forms.add("or-group:" + ("program" if "expr" in (p[0][0], p[2][0]) else "plain"))
            else:
                p, m, _ = rng.choice(good) if good else max(scored, key=lambda s: s[2])
                done, last = cur, m
                self.preds.append(p + (0,))
            self.pred_forms.add(p[1] + ":" + ("program" if p[0][0] == "expr" else "plain"))
            if p[2][0] == "expr":
                self.pred_forms.add("rhs:program")
        assert len(self.preds) <= MAX_PREDS and pred_nodes(self.preds) <= MAX_NODES

    def _padding(self, nodes):
        """An operand of exactly ``nodes`` (>= 1) nodes: a LEFT-nested sum of small columns (two values live)."""
        small = [c for s in ("a", "b") for c in self.cols[s] if c.bound is not None and c.bound <= 1000]
        tree = self.rng.choice(small).spec
        used = 1
        while used + 2 <= nodes:
            tree = ("+", tree, self.rng.choice(small).spec)
            used += 2
        if used < nodes:
            tree = ("abs", tree)
            self.kinds.add("abs")
        self.kinds.add("+")
        assert count_nodes(tree) == nodes
        return ("expr", tree)

    def _population_mask(self):
        return evaluate(self.preds, np.array(self.pa), np.array(self.pb)).tolist()

    # ---- what a test feeds the engine
    def candidates(self, n):
        """``n`` candidate pairs (every row pair of the population turns up once ``n`` is a few thousand)."""
        rng = np.random.default_rng(self.seed * 31 + n)
        return rng.integers(0, self.N_A, n).astype(np.int32), rng.integers(0, self.N_B, n).astype(np.int32)


MAX_ATTEMPTS = 8


def draw(seed, plain_only=False):
    """The draw of ``seed``: re-drawn while the reference overflows int64 or keeps a share of the population outside
    [2 %, 98 %].  ``draw.attempt`` tells how often."""
    for attempt in range(MAX_ATTEMPTS):
        try:
            d = Draw(seed, attempt, plain_only)
        except Int64Overflow:
            continue
        if 0.02 <= d.share <= 0.98:
            return d
    raise AssertionError(f"seed {seed}: no draw within the keep-share window in {MAX_ATTEMPTS} attempts")


#: the seeds and candidate counts of the GPU differential test (tests/test_select_semantics.py)
SIZES = (0, 1, 63, 64, 65, 2047, 2048, 2049)
BIG = 50_021
GPU_CASES = [(seed, n) for seed, n in enumerate(SIZES)] + [(seed, BIG) for seed in range(len(SIZES), 24)]
