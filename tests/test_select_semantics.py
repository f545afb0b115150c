"""The residual expression evaluator (`sel_load`, `sel_eval`, `sel_eval_prog` of select_kernels.hip.h) against a
plain-Python reference of its documented semantics (tests/_sel_ref.py).

CPU: the reference gives the golden rows of tests/golden/boolean_residuals.json through the plan's residuals and
agrees with the evaluator of tests/test_boolean_residuals.py; hand-written truth tables; the coverage of the seeded
generator over the seeds the GPU tests use.  GPU: generated predicate sets through `HipEngine.select`, bit for bit;
the limits at the Python wrapper and at the C ABI; every Arrow type `_Residuals._numeric` maps, through
`transpile` + `execute()`.  There is no tolerance anywhere: every step of the evaluator is one correctly rounded
binary64 operation or an exact integer one."""
import ctypes
import json
import math
import os

import numpy as np
import pytest

import _sel_ref as R

NAN, INF = math.nan, math.inf
GOLDEN_DOC = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "boolean_residuals.json")))
GOLDEN = GOLDEN_DOC["cases"] + GOLDEN_DOC["arith"]
COLS = ["chrom", "start", "end", "name", "score", "strand"]


# =========================================================================================== CPU: golden rows
class _GoldenSpecs:
    """A plan's residuals as `HipEngine.select` specs over numpy columns (left = side "a").  Strings under a
    comparison become ranks in one sorted dictionary shared by both operands (binary collation)."""

    def __init__(self, peaks, genes):
        self.rows = {"l": peaks, "r": genes}

    def _vals(self, side, col):
        return [r[COLS.index(col)] for r in self.rows[side]]

    def _is_str(self, t):
        return t[0] == "str" or (t[0] in ("l", "r") and t[1] in ("chrom", "name", "strand"))

    def _column(self, side, col, code=None):
        vals = self._vals(side, col)
        valid = np.array([v is not None for v in vals], np.uint8)
        if code is not None:
            data = np.array([code.get(v, 0) for v in vals], np.int32)
        elif col in ("chrom", "name", "strand"):
            data = np.zeros(len(vals), np.uint8)                        # only its validity is read
        elif any(isinstance(v, float) for v in vals):
            data = np.array([0.0 if v is None else v for v in vals], np.float64)
        else:
            data = np.array([0 if v is None else v for v in vals], np.int64)
        return ("a" if side == "l" else "b", data, valid)

    def _string_pair(self, kids):
        words = set()
        for t in kids:
            words |= {t[1]} if t[0] == "str" else {v for v in self._vals(t[0], t[1]) if v is not None}
        code = {w: k for k, w in enumerate(sorted(words))}
        return [("lit", code[t[1]]) if t[0] == "str" else self._column(t[0], t[1], code) for t in kids]

    def tree(self, t):
        if t[0] != "fn":
            return ("lit", t[1]) if t[0] in ("int", "float") else self._column(t[0], t[1])
        op, kids = t[1], [tuple(k) if k[0] != "fn" else k for k in t[2]]
        if op in R.CMP and any(self._is_str(k) for k in kids):
            return (op, *self._string_pair(kids))
        return (op, *[self.tree(k) for k in kids])

    def pred(self, res):
        ops = [(o.kind, o.value) for o in (res.lhs, res.rhs)]
        if res.op in ("isnull", "notnull", "istrue"):
            lhs = ("expr", self.tree(ops[0][1])) if ops[0][0] == "expr" else self.tree(ops[0])
            return lhs, res.op, ("lit", 0), res.group
        if any(self._is_str(o) for o in ops):
            lhs, rhs = self._string_pair(ops)
            return lhs, res.op, rhs, res.group
        lhs, rhs = (("expr", self.tree(o[1])) if o[0] == "expr" else self.tree(o) for o in ops)
        return lhs, res.op, rhs, res.group


@pytest.mark.parametrize("case", GOLDEN, ids=[f"{i}:{c['kind']}" for i, c in enumerate(GOLDEN)])
def test_the_reference_gives_the_golden_rows_through_the_plans_residuals(case):
    import test_boolean_residuals as T
    from giql_amd.transpile import build_plan

    plan = build_plan(case["query"], ["peaks", "genes"])
    peaks, genes = case["peaks"], case["genes"]
    specs = _GoldenSpecs(peaks, genes)
    pairs = [(i, j) for i, p in enumerate(peaks) for j, g in enumerate(genes) if T._overlap(p, g)]
    ia, ib = (np.array([p[k] for p in pairs], np.int64) for k in (0, 1))

    def mask(residuals, ia, ib):
        return R.evaluate([specs.pred(r) for r in residuals], ia, ib)

    if plan.kind == "INNER":
        keep = mask(plan.residuals, ia, ib)
        assert keep.tolist() == [T._holds(plan.residuals, peaks[i], genes[j]) for i, j in pairs]
        got = [[peaks[i][3], peaks[i][1], genes[j][3], genes[j][2]] for (i, j), k in zip(pairs, keep) if k]
    else:
        on = [r for r in plan.residuals if r.clause == "on"]
        where = [r for r in plan.residuals if r.clause == "where"]
        keep = mask(on, ia, ib)
        assert keep.tolist() == [T._holds(on, peaks[i], genes[j]) for i, j in pairs]
        matched = {i for (i, _j), k in zip(pairs, keep) if k}
        rows = np.arange(len(peaks))
        outer = mask(where, rows, np.zeros(len(peaks), np.int64))
        assert outer.tolist() == [T._holds(where, p, None) for p in peaks]
        got = [[p[3], p[1], p[4]] for i, p in enumerate(peaks) if outer[i] and ((i in matched) != (plan.kind == "ANTI"))]
    assert sorted(got, key=T._key) == case["rows"]


# =========================================================================================== CPU: truth tables
def _column_of(vals, dtype=None):
    """Python values (None = NULL) as a column spec of side "a"."""
    if dtype is None:
        dtype = np.float64 if any(isinstance(v, float) for v in vals) else np.int64
    data = np.array([0 if v is None else v for v in vals], dtype)
    if all(v is not None for v in vals):
        return ("a", data)
    return ("a", data, np.array([v is not None for v in vals], np.uint8))


def _table(kind, rows, n_args):
    """`rows` = [(arg, ..., expected)]: the node `kind` over columns holding the arguments, row by row."""
    cols = [_column_of([r[k] for r in rows]) for k in range(n_args)]
    rr = list(range(len(rows)))
    return R.values((kind, *cols), rr, rr), [r[n_args] for r in rows]


def _same(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        ok = (g is None and w is None) or (type(g) is type(w) and (g == w or (isinstance(w, float) and math.isnan(w) and math.isnan(g))))
        if ok and isinstance(w, float) and w == 0.0:
            ok = math.copysign(1, g) == math.copysign(1, w)
        assert ok, (k, g, w)


# booleans travel as the 0 / 1 the comparisons leave: T = 1, F = 0, NULL = None
KLEENE_AND = [(1, 1, True), (1, 0, False), (1, None, None), (0, 1, False), (0, 0, False), (0, None, False),
              (None, 1, None), (None, 0, False), (None, None, None)]
KLEENE_OR = [(1, 1, True), (1, 0, True), (1, None, True), (0, 1, True), (0, 0, False), (0, None, None),
             (None, 1, True), (None, 0, None), (None, None, None)]
KLEENE_NOT = [(1, False), (0, True), (None, None)]


def test_kleene_truth_tables():
    _same(*_table("and", KLEENE_AND, 2))
    _same(*_table("or", KLEENE_OR, 2))
    _same(*_table("not", KLEENE_NOT, 1))
    _same(*_table("isnull", [(1, False), (0, False), (None, True)], 1))
    _same(*_table("notnull", [(1, True), (0, True), (None, False)], 1))
    # three arguments; a filter keeps TRUE only
    _same(*_table("and", [(1, 1, None, None), (1, None, 0, False), (1, 1, 1, True)], 3))
    _same(*_table("or", [(0, 0, None, None), (0, None, 1, True), (0, 0, 0, False)], 3))
    col = _column_of([1, 0, None])
    assert R.evaluate([(("expr", ("not", col)), "istrue", ("lit", 0))], np.arange(3), np.arange(3)).tolist() == [False, True, False]
    assert R.evaluate([(col, "=", ("lit", 1), 1), (col, "isnull", ("lit", 0), 1), (col, "!=", ("lit", 7))],
                      np.arange(3), np.arange(3)).tolist() == [True, False, False]


LEAST_ROWS = [(3, 5, 3), (5, 3, 3), (None, 5, 5), (5, None, 5), (None, None, None), (-7, -7, -7)]
GREATEST_ROWS = [(3, 5, 5), (5, 3, 5), (None, 5, 5), (5, None, 5), (None, None, None), (-7, -7, -7)]


def test_least_and_greatest_skip_nulls():
    _same(*_table("least", LEAST_ROWS, 2))
    _same(*_table("greatest", GREATEST_ROWS, 2))
    _same(*_table("least", [(None, None, 4, 4), (9, None, 4, 4), (None, None, None, None), (2, 8, None, 2)], 3))
    # a float argument makes the result a float; where it is NULL the integer stays an integer
    a, b = _column_of([3, 3, None]), _column_of([2.5, None, 2.5])
    _same(R.values(("least", a, b), [0, 1, 2], [0, 1, 2]), [2.5, 3, 2.5])
    _same(R.values(("greatest", a, b), [0, 1, 2], [0, 1, 2]), [3.0, 3, 2.5])
    # one argument is the argument
    _same(R.values(("greatest", a), [0, 2], [0, 2]), [3, None])


def test_division_is_binary64_and_null_on_a_zero_divisor():
    rows = [(7, 2, 3.5), (7, 0, None), (7.0, 0.0, None), (7.0, -0.0, None), (0, 5, 0.0), (None, 2, None), (7, None, None),
            (-1, 3, -1 / 3), (2**53 + 1, 1, 2.0**53), (1, 2**53 + 1, 1 / 2.0**53), (INF, INF, NAN), (0.0, INF, 0.0)]
    for a, b, want in rows:        # (one column per value: an integer stays an integer column)
        _same(R.values(("/", _column_of([a]), _column_of([b])), [0], [0]), [want])


def test_integers_stay_exact_and_a_float_beside_them_rounds():
    big = 2**53 + 1
    one = lambda tree: R.values(tree, [0], [0])[0]
    I, F = (lambda v: _column_of([v], np.int64)), (lambda v: _column_of([v], np.float64))
    assert one(("=", I(big), F(2.0**53))) is True              # the integer is cast: float(2^53 + 1) = 2^53
    assert one(("=", I(big), I(2**53))) is False               # between integers the comparison is exact
    assert one(("<", I(2**53), I(big))) is True
    assert one((">", I(R.I64_MAX), F(2.0**63))) is False and one(("=", I(R.I64_MAX), F(2.0**63))) is True
    assert one(("<", I(R.I64_MIN), I(R.I64_MIN + 1))) is True
    assert one(("*", _column_of([2**31 - 1], np.int32), _column_of([-(2**31)], np.int32))) == -(2**31) * (2**31 - 1)
    assert one(("+", I(big), ("lit", 1))) == 2**53 + 2 and one(("+", I(big), ("lit", 1.0))) == 2.0**53   # cast, then a tie to even
    assert one(("-", ("neg", I(big)), ("lit", 0))) == -big and one(("abs", I(-big))) == big
    assert one(("*", I(3), F(0.5))) == 1.5 and one(("+", I(3), F(None))) is None
    assert one(("=", _column_of([0.1], np.float32), ("lit", 0.1))) is False
    assert one(("=", _column_of([0.1], np.float32), ("lit", R.F32_TENTH))) is True
    assert one(("=", _column_of([255], np.uint8), ("lit", 255))) is True
    assert one(("=", F(0.0), F(-0.0))) is True
    with pytest.raises(R.Int64Overflow):
        one(("+", I(R.I64_MAX), ("lit", 1)))
    with pytest.raises(R.Int64Overflow):
        one(("neg", I(R.I64_MIN)))
    with pytest.raises(R.Int64Overflow):
        one(("*", I(2**32), I(2**31)))


NAN_ROWS = [("=", False), ("!=", True), ("<", False), ("<=", False), (">", False), (">=", False)]


def test_nan_follows_ieee():
    """Unspecified upstream (its two engines disagree); IEEE here, DESIGN section 4b."""
    F = lambda v: _column_of([v], np.float64)
    one = lambda tree: R.values(tree, [0], [0])[0]
    for op, want in NAN_ROWS:
        assert one((op, F(NAN), F(1.0))) is want and one((op, F(1.0), F(NAN))) is want and one((op, F(NAN), F(NAN))) is want
        assert one((op, F(NAN), _column_of([1], np.int64))) is want
        assert R.evaluate([(F(NAN), op, ("lit", 1.0))], [0], [0]).tolist() == [want]
    assert R.evaluate([(("expr", ("+", F(NAN), ("lit", 1))), "istrue", ("lit", 0))], [0], [0]).tolist() == [True]   # NaN IS TRUE
    assert one(("not", F(NAN))) is False and one(("and", F(NAN), ("lit", 1))) is True
    assert one(("isnull", F(NAN))) is False and math.isnan(one(("/", F(NAN), ("lit", 2))))
    # LEAST / GREATEST fold with < / >: a NaN stays only as the first non-NULL argument
    assert math.isnan(one(("least", F(NAN), F(1.0)))) and one(("least", F(1.0), F(NAN))) == 1.0
    assert math.isnan(one(("greatest", F(NAN), F(1.0)))) and one(("greatest", F(None), F(1.0), F(NAN))) == 1.0


# =========================================================================================== CPU: generator coverage
@pytest.fixture(scope="module")
def draws():
    return {seed: R.draw(seed) for seed in sorted({s for s, _n in R.GPU_CASES})}


def test_the_generator_reaches_every_case_over_the_gpu_seeds(draws):
    ds = list(draws.values())
    union = lambda attr: set().union(*[getattr(d, attr) for d in ds])
    assert union("kinds") == set(R.KINDS) and set(R.KINDS) == set(_engine_xops())
    assert union("depths") == {(k, d) for k in ("arith", "bool") for d in range(1, R.MAX_LIVE + 1)}
    pairs = {(x, y) for x in R.TYPES for y in R.TYPES}
    assert union("cmp_pairs") == pairs and union("arith_pairs") == pairs
    assert union("edges") == R.ALL_EDGES, sorted(map(str, R.ALL_EDGES - union("edges")))
    assert union("nullness") == {"none", "some", "all"} and union("lit_kinds") == {"int", "float"}
    assert union("arities") >= {(op, k) for op in R.NARY for k in (1, 2, 3, 4)}
    forms = union("pred_forms")
    assert forms >= {"or-group:program", "or-group:plain", "rhs:program", "istrue:program", "isnull:program", "notnull:program",
                     "isnull:plain", "notnull:plain"} | {f"{op}:{w}" for op in R.CMP for w in ("plain", "program")}, forms
    assert max(d.n_nodes for d in ds) == R.MAX_NODES and max(len(d.preds) for d in ds) == R.MAX_PREDS
    assert any(sum(p[0][0] == "expr" for p in d.preds) + sum(p[2][0] == "expr" for p in d.preds) >= 4 for d in ds)
    # the window and the cap are conditions the generator meets
    assert all(0.02 <= d.share <= 0.98 for d in ds)
    assert sum(d.attempt > 0 for d in ds) * 2 <= len(ds) and sum(d.attempt for d in ds) * 2 <= len(ds)
    # every tree obeys the limits it is flattened under, and INT64_MIN sits under comparisons only
    for d in ds:
        assert R.pred_nodes(d.preds) == d.n_nodes <= R.MAX_NODES
        for p in d.preds:
            for o in (p[0], p[2]):
                if o[0] == "expr":
                    assert R.live_values(o) <= R.MAX_LIVE
                    _min_under_comparisons_only(o[1], d, False)
    # the cases the GPU test feeds: both kept and dropped candidates wherever there are a few
    for seed, n in R.GPU_CASES:
        ia, ib = draws[seed].candidates(n)
        want = R.evaluate(draws[seed].preds, ia, ib)
        assert n < 63 or 0 < want.sum() < n, (seed, n)
    # the big product is there: two int32 columns whose product passes 2^61
    d = ds[0]
    a, b = (next(c for c in d.cols[s] if c.name == "i32_big").data.astype(object) for s in ("a", "b"))
    assert max(abs(int(x) * int(y)) for x in a for y in b) > 2**61


def _engine_xops():
    from giql_amd.engine import HipEngine

    return HipEngine._XOPS


def _min_under_comparisons_only(tree, d, under_cmp):
    if tree[0] in ("a", "b"):
        if tree[0] != "lit" and tree[1].dtype == np.int64 and (tree[1] == R.I64_MIN).any():
            ok = np.ones(len(tree[1]), bool) if len(tree) < 3 else tree[2].astype(bool)
            assert under_cmp or not (tree[1][ok] == R.I64_MIN).any()
        return
    if tree[0] == "lit":
        return
    for c in tree[1:]:
        _min_under_comparisons_only(c, d, tree[0] in R.CMP)


def test_the_generator_is_a_function_of_its_seed():
    a, b = R.draw(5), R.draw(5)
    assert repr(_strip(a.preds)) == repr(_strip(b.preds)) and a.share == b.share
    assert all(np.array_equal(x.data, y.data, equal_nan=x.data.dtype.kind == "f") for x, y in zip(a.cols["a"], b.cols["a"]))


def _strip(t):
    """A spec with its arrays replaced by their bytes (for comparing two draws)."""
    if isinstance(t, np.ndarray):
        return t.tobytes()
    return tuple(_strip(x) for x in t) if isinstance(t, (tuple, list)) else t


def test_node_and_live_value_counts_match_the_flattening():
    x = ("a", np.zeros(1, np.int32))
    assert R.count_nodes(("+", x, ("+", x, ("+", x, x)))) == 7 and R.live_values(("+", x, ("+", x, ("+", x, x)))) == 4
    assert R.count_nodes(("+", ("+", ("+", x, x), x), x)) == 7 and R.live_values(("+", ("+", ("+", x, x), x), x)) == 2
    assert R.count_nodes(("least", x)) == 1 and R.count_nodes(("least", x, x, x, x)) == 7 and R.live_values(("least", x, x, x, x)) == 2
    assert R.count_nodes(("not", ("isnull", x))) == 3 and R.live_values(("or", ("isnull", x), ("and", ("isnull", x), ("<", x, x)))) == 4


# =========================================================================================== GPU
def _torch():
    import torch

    return torch


@pytest.fixture(scope="module")
def eng():
    from giql_amd.engine import HipEngine

    assert _torch().cuda.is_available(), "GPU tests need a HIP device"
    e = HipEngine(0)
    yield e
    e.close()


class _Dev:
    """Specs over numpy arrays -> the same specs over device tensors (one upload per array); `rows` re-addresses a
    side by the candidate index: its columns are gathered by the ids the call then leaves out."""

    def __init__(self, rows=None):
        self.cache, self.rows = {}, rows or {}

    def tensor(self, side, x):
        key = (side, id(x))
        if key not in self.cache:
            y = x[self.rows[side]] if side in self.rows else x
            self.cache[key] = (x, _torch().from_numpy(np.ascontiguousarray(y)).cuda())
        return self.cache[key][1]

    def spec(self, t):
        if t[0] in ("a", "b"):
            return (t[0], *[self.tensor(t[0], x) for x in t[1:]])
        if t[0] == "lit":
            return t
        return (t[0], *[self.spec(c) for c in t[1:]])

    def preds(self, preds):
        return [(self.spec(p[0]), p[1], self.spec(p[2]), *p[3:]) for p in preds]


def _select_and_compare(eng, preds, ia, ib, n_a, n_b, mode=0, want=("a", "b"), keep=None):
    """`eng.select` against the reference mask; mode bit 0 / 1 = leave idx_a / idx_b out ("the candidate index")."""
    torch = _torch()
    n = len(ia)
    if keep is None:
        keep = R.evaluate(preds, ia, ib)
    rows = {s: x.astype(np.int64) for s, x, bit in (("a", ia, 1), ("b", ib, 2)) if mode & bit}
    dev = _Dev(rows)
    ida = None if mode & 1 else torch.from_numpy(ia).cuda()
    idb = None if mode & 2 else torch.from_numpy(ib).cuda()
    ga, gb = eng.select(dev.preds(preds), idx_a=ida, idx_b=idb, n=n, n_rows_a=n if mode & 1 else n_a,
                        n_rows_b=n if mode & 2 else n_b, want=want)
    cand = np.arange(n, dtype=np.int32)
    for got, side, ids, bit in ((ga, "a", ia, 1), (gb, "b", ib, 2)):
        if side not in want:
            assert got is None
            continue
        exp = (cand if mode & bit else ids)[keep]
        got = got.cpu().numpy()
        if not np.array_equal(got, exp):
            first = int(np.nonzero(np.resize(got, n) != np.resize(exp, n))[0][0]) if len(got) and len(exp) else 0
            raise AssertionError(f"side {side}: kept {len(got)} candidates, the reference {len(exp)}; first difference at "
                                 f"output {first}")
    return keep


WANTS = (("a", "b"), ("a",), ("b",))


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(R.GPU_CASES)), ids=[f"seed{s}-n{n}" for s, n in R.GPU_CASES])
def test_generated_predicates_match_the_reference(eng, k):
    seed, n = R.GPU_CASES[k]
    d = R.draw(seed)
    ia, ib = d.candidates(n)
    keep = _select_and_compare(eng, d.preds, ia, ib, d.N_A, d.N_B, mode=0, want=WANTS[k % 3])
    # the same call with one side, the other, or both addressed by the candidate index, and the other `want`s
    _select_and_compare(eng, d.preds, ia, ib, d.N_A, d.N_B, mode=1 + k % 3, want=WANTS[(k + 1) % 3], keep=keep)
    _select_and_compare(eng, d.preds, ia, ib, d.N_A, d.N_B, mode=1 + (k + 1) % 3, want=WANTS[(k + 2) % 3], keep=keep)
    print(f"seed {seed} n {n}: {len(d.preds)} predicates, {d.n_nodes} nodes, kept {int(keep.sum())}")


# one clause per predicate, to tell which one of a failing set diverges (a debugging aid that also runs each
# predicate of every big draw on its own: no other clause can hide its error)
@pytest.mark.gpu
@pytest.mark.parametrize("seed", [s for s, n in R.GPU_CASES if n == R.BIG][::3])
def test_each_generated_clause_on_its_own(eng, seed):
    d = R.draw(seed)
    ia, ib = d.candidates(4099)
    for j, clause in enumerate(R.clauses(d.preds)):
        try:
            _select_and_compare(eng, clause, ia, ib, d.N_A, d.N_B)
        except AssertionError as e:
            raise AssertionError(f"seed {seed} clause {j} {_describe(clause)}: {e}") from None


def _describe(t):
    if isinstance(t, np.ndarray):
        return f"{t.dtype}[{len(t)}]"
    return "(" + " ".join(_describe(x) for x in t) + ")" if isinstance(t, (tuple, list)) else repr(t)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n", [(40, 2049), (41, R.BIG), (42, R.BIG)])
def test_both_template_instances_give_the_same_ids(eng, seed, n):
    # only plain predicates: k_select_count<false>; the same beside one program that is always TRUE: <true>
    d = R.draw(seed, plain_only=True)
    assert d.n_nodes == 0 and len(d.preds) < R.MAX_PREDS
    ia, ib = d.candidates(n)
    keep = _select_and_compare(eng, d.preds, ia, ib, d.N_A, d.N_B)
    always = (("expr", ("+", ("lit", 1), ("lit", 1))), "=", ("lit", 2))
    for preds in (d.preds + [always], [always] + d.preds):
        _select_and_compare(eng, preds, ia, ib, d.N_A, d.N_B, keep=keep)
    assert 0 < keep.sum() < n


@pytest.mark.gpu
def test_hand_written_rows_on_the_gpu(eng):
    """The truth tables above, through the kernel: every row of every table is one candidate."""
    def run(tree, rows, n_args, istrue=True):
        cols = [_column_of([r[k] for r in rows]) for k in range(n_args)]
        ids = np.arange(len(rows), dtype=np.int32)
        for op in ("istrue", "isnull", "notnull"):
            _select_and_compare(eng, [(("expr", (tree, *cols)), op, ("lit", 0))], ids, ids, len(rows), len(rows))

    run("and", KLEENE_AND, 2)
    run("or", KLEENE_OR, 2)
    run("not", KLEENE_NOT, 1)
    ids = lambda n: np.arange(n, dtype=np.int32)
    for kind, rows in (("least", LEAST_ROWS), ("greatest", GREATEST_ROWS)):
        for op in R.CMP:
            a, b = _column_of([r[0] for r in rows]), _column_of([r[1] for r in rows])
            _select_and_compare(eng, [(("expr", (kind, a, b)), op, ("lit", 5))], ids(len(rows)), ids(len(rows)), len(rows), len(rows))
            _select_and_compare(eng, [(("expr", (kind, a, b)), "isnull", ("lit", 0))], ids(len(rows)), ids(len(rows)), len(rows), len(rows))
    # division by 0 and -0.0; 2^53 + 1 = 2.0^53; the NaN rows
    num = _column_of([7, 7, 0, 2**53 + 1, -1], np.int64)
    den = _column_of([0.0, -0.0, 5.0, 1.0, 3.0], np.float64)
    for op in ("isnull", "notnull"):
        keep = _select_and_compare(eng, [(("expr", ("/", num, den)), op, ("lit", 0))], ids(5), ids(5), 5, 5)
        assert keep.tolist() == [op == "isnull"] * 2 + [op != "isnull"] * 3
    keep = _select_and_compare(eng, [(_column_of([2**53 + 1, 2**53 + 1], np.int64), "=", _column_of([2.0**53, 2.0**53 + 2]))],
                               ids(2), ids(2), 2, 2)
    assert keep.tolist() == [True, False]
    nan = _column_of([NAN, 1.0, NAN], np.float64)
    other = _column_of([1.0, NAN, NAN], np.float64)
    for op, want in NAN_ROWS:
        assert _select_and_compare(eng, [(nan, op, other)], ids(3), ids(3), 3, 3).tolist() == [want] * 3
        assert _select_and_compare(eng, [(("expr", (op, nan, other)), "istrue", ("lit", 0))], ids(3), ids(3), 3, 3).tolist() == [want] * 3
    assert _select_and_compare(eng, [(("expr", ("+", nan, ("lit", 0))), "istrue", ("lit", 0))], ids(3), ids(3), 3, 3).tolist() == [True] * 3


def _product_case(n, seed=7):
    """Two int32 columns whose products reach 2^62, and an int64 column that holds each product or misses it by one:
    an evaluator that takes the product through a double (53 bits) cannot tell the two apart."""
    rng = np.random.default_rng(seed)
    sign = lambda: rng.choice(np.array([-1, 1], np.int64), n)
    p = (rng.integers(1518500250, 2**31 - 1, n) * sign()).astype(np.int32)
    q = (rng.integers(1518500250, 2**31 - 1, n) * sign()).astype(np.int32)
    p[:4], q[:4] = [2**31 - 1, -(2**31), -(2**31), 3], [2**31 - 1, -(2**31), 2**31 - 1, -5]
    delta = rng.integers(-1, 2, n)
    z = p.astype(np.int64) * q.astype(np.int64) + delta
    return p, q, z, delta


def test_the_product_case_needs_more_than_53_bits():
    p, q, z, delta = _product_case(4096)
    exact = [int(x) * int(y) for x, y in zip(p, q)]
    assert max(map(abs, exact)) == 2**62 and min(map(abs, exact[4:])) > 2**61
    assert sum(int(float(e)) != e for e in exact) > 3000            # a double would have rounded most of them
    ids = np.arange(4096)
    keep = R.evaluate([(("expr", ("*", ("a", p), ("b", q))), "=", ("a", z))], ids, ids)
    assert keep.tolist() == (delta == 0).tolist() and 1000 < keep.sum() < 2000


@pytest.mark.gpu
def test_int32_products_stay_64_bit_on_the_gpu(eng):
    # named regression case for "integer MUL routed through double": no generated comparison depends on the last
    # bits of a 2^62 product, these do
    n = R.BIG
    p, q, z, delta = _product_case(n)
    ids = np.arange(n, dtype=np.int32)
    P, Q, Z = ("a", p), ("b", q), ("a", z)
    for preds, want in (
            ([(("expr", ("*", P, Q)), "=", Z)], delta == 0),
            ([(("expr", ("-", ("*", P, Q), Z)), ">", ("lit", 0))], delta < 0),
            ([(("expr", ("and", ("<=", ("*", Q, P), Z), ("!=", ("neg", ("*", P, Q)), ("neg", Z)))), "istrue", ("lit", 0))], delta > 0)):
        keep = _select_and_compare(eng, preds, ids, ids, n, n)
        assert np.array_equal(keep, want)


# ---- limits at the Python wrapper
def _sum_of(n_leaves, leaf):
    tree = leaf
    for _ in range(n_leaves - 1):
        tree = ("+", tree, leaf)
    return tree


@pytest.mark.gpu
def test_wrapper_limits_256_nodes_and_12_live_values(eng):
    from giql_amd._lib import GiqlHipError

    torch = _torch()
    col = np.arange(-20, 20, dtype=np.int32)
    leaf = ("a", torch.from_numpy(col).cuda())
    kw = dict(n=40, n_rows_a=40, want=("a",))
    full = ("abs", _sum_of(128, leaf))                                   # 255 + 1 nodes
    assert R.count_nodes(("abs", _sum_of(128, ("a", col)))) == 256
    got = eng.select([(("expr", full), ">", ("lit", 1280))], **kw)[0]
    assert np.array_equal(got.cpu().numpy(), np.nonzero(np.abs(col.astype(np.int64) * 128) > 1280)[0])
    with pytest.raises(ValueError, match="256 expression nodes"):
        eng.select([(("expr", full), ">", ("expr", ("lit", 1280)))], **kw)      # 257
    # twelve values live fit, thirteen do not: arithmetic ...
    def nested(levels, op, term, last):
        tree = last
        for _ in range(levels):
            tree = (op, term, tree)
        return tree
    ok = nested(11, "+", leaf, leaf)
    assert R.live_values(nested(11, "+", ("a", col), ("a", col))) == 12
    got = eng.select([(("expr", ok), ">", ("lit", 0))], **kw)[0]
    assert np.array_equal(got.cpu().numpy(), np.nonzero(col > 0)[0])
    with pytest.raises(GiqlHipError, match="deeper than 12"):
        eng.select([(("expr", nested(12, "+", leaf, leaf)), ">", ("lit", 0))], **kw)
    # ... and a boolean program
    term, last = ("notnull", leaf), (">", leaf, ("lit", 3))
    assert R.live_values(nested(10, "and", ("notnull", ("a", col)), (">", ("a", col), ("lit", 3)))) == 12
    got = eng.select([(("expr", nested(10, "and", term, last)), "istrue", ("lit", 0))], **kw)[0]
    assert np.array_equal(got.cpu().numpy(), np.nonzero(col > 3)[0])
    with pytest.raises(GiqlHipError, match="deeper than 12"):
        eng.select([(("expr", nested(11, "and", term, last)), "istrue", ("lit", 0))], **kw)
    # the context still answers
    assert int(eng.select([(leaf, ">", ("lit", 3))], **kw)[0].shape[0]) == int((col > 3).sum())


# ---- limits at the C ABI: argument checks that return before any launch
@pytest.mark.gpu
def test_c_abi_refuses_malformed_programs_and_still_answers(eng):
    from giql_amd import _lib

    torch = _torch()
    L, n = eng._L, 8
    col = torch.arange(n, dtype=torch.int32, device="cuda")
    out = torch.full((n,), -1, dtype=torch.int32, device="cuda")

    def lit(v):
        o = _lib.COperand()
        o.side, o.lit_i = _lib.SIDE_LIT, v
        return o

    def node(kind):
        o = _lib.COperand()
        o.side = kind
        return o

    def program(first, count):
        o = _lib.COperand()
        o.side, o.lit_i, o.type = _lib.SIDE_EXPR, first, count
        return o

    def column():
        o = _lib.COperand()
        o.side, o.type, o.data = _lib.SIDE_A, _lib.T_I32, col.data_ptr()
        return o

    def call(lhs, nodes, op=_lib.OPS[">"], group=0, n_nodes=None):
        preds = (_lib.CPred * 1)()
        preds[0].lhs, preds[0].rhs, preds[0].op, preds[0].group = lhs, lit(3), op, group
        c_nodes = (_lib.COperand * len(nodes))(*nodes) if nodes else None
        kept = ctypes.c_int64(-5)
        rc = L.giql_hip_select_expr_dev(eng._h, preds, 1, c_nodes, len(nodes) if n_nodes is None else n_nodes, None, n, None, 0,
                                        n, out.data_ptr(), None, ctypes.byref(kept), None)
        return rc, (L.giql_hip_last_error() or b"").decode(), int(kept.value)

    ADD = eng._XOPS["+"]
    refusals = [
        ("an operator with too few values", program(0, 2), [lit(1), node(ADD)], {}, "predicate 0 lhs: malformed expression"),
        ("two values left", program(0, 2), [lit(1), lit(2)], {}, "predicate 0 lhs: malformed expression"),
        ("an unknown node kind", program(0, 2), [lit(1), node(99)], {}, "predicate 0 lhs: expression node kind 99"),
        ("first + count past n_nodes", program(0, 2), [lit(1)], {}, "expression nodes [0, 2) outside the 1 given"),
        ("first past n_nodes", program(1, 1), [lit(1)], {}, "expression nodes [1, 2) outside the 1 given"),
        ("no nodes at all", program(0, 1), [], {}, "expression nodes [0, 1) outside the 0 given"),
        ("a negative group", column(), [], {"group": -1}, "predicate 0: group -1"),
    ]
    for what, lhs, nodes, kw, message in refusals:
        rc, err, _kept = call(lhs, nodes, **kw)
        assert rc == _lib.GIQL_ERR_INVALID, what
        assert message in err, (what, err)
    assert bool((out == -1).all())                                  # nothing was launched, nothing written
    # a valid program and a valid plain call on the same context
    rc, err, kept = call(program(0, 3), [column(), lit(1), node(ADD)])           # col + 1 > 3
    assert (rc, kept) == (_lib.GIQL_OK, 5), err
    assert out.cpu().tolist() == [3, 4, 5, 6, 7, -1, -1, -1]
    rc, err, kept = call(column(), [])
    assert (rc, kept) == (_lib.GIQL_OK, 4), err


# ---- every Arrow type _Residuals._numeric maps, through transpile + execute()
ARROW_KINDS = ["int8", "int16", "uint8", "uint16", "uint32", "int64", "uint64", "float16", "float32", "float64", "bool",
               "dictionary", "chunked", "sliced"]


def _arrow_column(kind, n, rng):
    """(arrow column of n rows, its values as Python numbers / None)."""
    import pyarrow as pa

    null = rng.random(n) < 0.2
    ints = {"int8": (-128, 127, pa.int8()), "int16": (-32768, 32767, pa.int16()), "uint8": (0, 255, pa.uint8()),
            "uint16": (0, 65535, pa.uint16()), "uint32": (2**31, 2**32 - 1, pa.uint32()),
            "int64": (-(2**62), 2**62, pa.int64()), "uint64": (2**62, 2**63 - 2, pa.uint64()),
            "dictionary": (-3, 3, pa.int32()), "chunked": (-3, 3, pa.int32()), "sliced": (-3, 3, pa.int64())}
    if kind in ints:
        lo, hi, typ = ints[kind]
        # few distinct values, the ends of the range among them: comparisons between two columns hold often enough
        pool = [lo, hi, lo + 1, hi - 1, (lo + hi) // 2] if hi - lo > 8 else list(range(lo, hi + 1))
        vals = [None if z else pool[int(rng.integers(0, len(pool)))] for z in null]
        if kind == "sliced":
            return pa.array([7, None, 9] + vals, typ).slice(3), vals
        arr = pa.array(vals, typ)
        if kind == "dictionary":
            return arr.dictionary_encode(), vals
        if kind == "chunked":
            cut = n // 3
            return pa.chunked_array([arr[:cut], arr[cut:cut], arr[cut:]]), vals
        return arr, vals
    if kind == "bool":
        vals = [None if z else bool(rng.integers(0, 2)) for z in null]
        return pa.array(vals, pa.bool_()), vals
    dt = {"float16": np.float16, "float32": np.float32, "float64": np.float64}[kind]
    pool = np.array([0.1, -2.5, 0.0, 3.0, 65504.0 if kind == "float16" else 1e30, 1 / 3], dt)
    data = pool[rng.integers(0, len(pool), n)]
    arr = pa.array(data, mask=null)
    assert str(arr.type) == {"float16": "halffloat", "float32": "float", "float64": "double"}[kind]
    return arr, [None if z else float(x) for x, z in zip(data, null)]


def _numeric_spec(side, vals):
    """Python numbers / None as a reference column: the value of the column, whatever Arrow type carried it."""
    valid = np.array([v is not None for v in vals], np.uint8)
    if any(isinstance(v, float) for v in vals):
        return (side, np.array([0.0 if v is None else v for v in vals], np.float64), valid)
    return (side, np.array([0 if v is None else int(v) for v in vals], np.int64), valid)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ARROW_KINDS)
def test_execute_reads_every_arrow_type_in_a_predicate(kind):
    import pyarrow as pa

    from giql_amd.execute import execute
    from giql_amd.transpile import transpile

    k = ARROW_KINDS.index(kind)
    rng = np.random.default_rng(500 + k)
    other = ARROW_KINDS[(k + 5) % len(ARROW_KINDS)]
    tables, vals, rows = {}, {}, {}
    for name, n, col, ckind in (("ta", 300, "v", kind), ("tb", 260, "w", other)):
        start = rng.integers(0, 3000, n)
        end = start + rng.integers(1, 300, n)
        chrom = rng.integers(1, 3, n)
        arr, vals[name] = _arrow_column(ckind, n, rng)
        rows[name] = (chrom, start, end)
        tables[name] = pa.table({"chrom": pa.array([f"chr{c}" for c in chrom]), "start": pa.array(start, pa.int32()),
                                 "end": pa.array(end, pa.int32()), "name": pa.array([f"{name}{i}" for i in range(n)]), col: arr})
    (ca, sa, ea), (cb, sb, eb) = rows["ta"], rows["tb"]
    hit = (ca[:, None] == cb[None, :]) & (sa[:, None] < eb[None, :]) & (ea[:, None] > sb[None, :])
    ia, ib = np.nonzero(hit)
    V, W = _numeric_spec("a", vals["ta"]), _numeric_spec("b", vals["tb"])
    base = "SELECT a.name, b.name AS b_name FROM ta a JOIN tb b ON a.interval INTERSECTS b.interval AND "
    seen = 0
    for j, op in enumerate(R.CMP):
        sql_op = "<>" if op == "!=" else op
        conditions = [(f"a.v {sql_op} b.w", [(V, op, W)])]
        if j % 2 == k % 2:
            conditions.append((f"a.v + 1 {sql_op} b.w", [(("expr", ("+", V, ("lit", 1))), op, W)]))
        if j == 0:
            conditions.append(("a.v IS NULL", [(V, "isnull", ("lit", 0))]))
            conditions.append((f"(a.v + 1 {sql_op} b.w OR a.v IS NULL)", [(("expr", ("+", V, ("lit", 1))), op, W, 1), (V, "isnull", ("lit", 0), 1)]))
        for text, preds in conditions:
            keep = R.evaluate(preds, ia, ib)
            out = execute(transpile(base + text, tables=["ta", "tb"], dialect="hip"), tables)
            got = sorted(zip(out.column("name").to_pylist(), out.column("b_name").to_pylist()))
            want = sorted((f"ta{i}", f"tb{j_}") for i, j_ in zip(ia[keep], ib[keep]))
            assert got == want, (kind, other, text, len(got), len(want))
            seen += 0 < len(want) < len(ia)
    assert seen >= 4 and len(ia) > 500


@pytest.mark.gpu
def test_execute_refuses_what_a_predicate_cannot_read():
    import pyarrow as pa

    from giql_amd.execute import execute
    from giql_amd.transpile import transpile

    def table(name, col, arr):
        n = len(arr)
        return pa.table({"chrom": pa.array(["chr1"] * n), "start": pa.array(np.arange(n) * 10, pa.int32()),
                         "end": pa.array(np.arange(n) * 10 + 25, pa.int32()), "name": pa.array([f"{name}{i}" for i in range(n)]),
                         col: arr})

    base = "SELECT a.name, b.name AS b_name FROM ta a JOIN tb b ON a.interval INTERSECTS b.interval AND "
    w = pa.array(np.arange(6), pa.int64())
    t = {"ta": table("ta", "v", pa.array([1, 2**63, 3, 4, 5, 6], pa.uint64())), "tb": table("tb", "w", w)}
    with pytest.raises(ValueError, match="uint64 values beyond int64"):
        execute(transpile(base + "a.v > b.w", tables=["ta", "tb"], dialect="hip"), t)
    t["ta"] = table("ta", "v", pa.array([1, 2**63 - 1, 3, 4, 5, 6], pa.uint64()))        # the largest that fits
    out = execute(transpile(base + "a.v > b.w", tables=["ta", "tb"], dialect="hip"), t)
    assert out.num_rows > 0
    t["ta"] = table("ta", "v", pa.array(np.arange(6), pa.int32()).cast(pa.date32()))
    with pytest.raises(ValueError, match="is not supported in a dialect='hip' predicate"):
        execute(transpile(base + "a.v > b.w", tables=["ta", "tb"], dialect="hip"), t)
    with pytest.raises(ValueError, match="is not supported in a dialect='hip' predicate expression"):
        execute(transpile(base + "a.v + 1 > b.w", tables=["ta", "tb"], dialect="hip"), t)
