"""Aggregates of per-pair expressions over a join's pairs per left row on the GPU: ``HipEngine.pair_aggregate`` with
``("expr", tree)`` sources (``giql_hip_pair_expr_agg_dev``) against tests/_pair_expr_agg_ref.py, on pair arrays
alone -- no join runs here.

Shapes: ``MAGG_TILE = 256`` positions per reduction block, 64 tiles per fold step, ``RS_TILE = 4096`` pairs per sort
tile, 8-bit sort digits (a pass is added at 256 and 65,536 rows), wave 64.

Exactness: counts, integer results and MIN / MAX compare with ``==`` (the interpreter and the reference apply the
same binary64 operations to a pair, so a pair's value has the same bits); AVG of an integer tree too (|sum| < 2^53
here).  A float SUM over k non-NULL values may differ from ``fsum`` by at most k * 2^-52 * sum|x_i| and a float AVG by
that over k plus one ulp of the result -- the bound of tests/test_pair_agg_gpu.py, derived there."""
import math

import numpy as np
import pytest

import _pair_agg_ref as R
import _pair_expr_agg_ref as X

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TILE, FOLD, RS_TILE = 256, 64, 4096
FIVE = ("COUNT", "SUM", "MIN", "MAX", "AVG")


@pytest.fixture(scope="module")
def eng():
    from giql_amd.engine import HipEngine

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    e = HipEngine(0)
    yield e
    e.close()


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _to_dev(tree, memo):
    """A numpy tree of tests/_expr_ref.py as the engine's: every array uploaded once."""
    if tree[0] in ("a", "b"):
        out = [tree[0]]
        for arr in tree[1:]:
            if arr is None:
                out.append(None)
                continue
            if id(arr) not in memo:
                memo[id(arr)] = _dev(arr.astype(np.uint8) if arr.dtype == bool else arr)
            out.append(memo[id(arr)])
        return tuple(out)
    if tree[0] in ("lit", "null"):
        return tree
    return (tree[0],) + tuple(_to_dev(c, memo) for c in tree[1:])


class Tables:
    """Seeded columns of an A and a B table: interval-like integers, scores that are multiples of 1/4, a column with
    NULLs on each side, a divisor with zeros."""

    def __init__(self, seed, n_a, n_b):
        r = np.random.default_rng(seed)
        self.n_a, self.n_b = n_a, n_b
        self.a_start = r.integers(0, 100_000, n_a).astype(np.int32)
        self.a_end = (self.a_start + r.integers(1, 5_000, n_a)).astype(np.int32)
        self.b_start = r.integers(0, 100_000, n_b).astype(np.int32)
        self.b_end = (self.b_start + r.integers(1, 5_000, n_b)).astype(np.int64)
        self.a_score = (r.integers(-400, 400, n_a) / 4.0).astype(np.float64)
        self.b_score = (r.integers(-400, 400, n_b) / 4.0).astype(np.float32)
        self.b_div = r.integers(-2, 3, n_b).astype(np.int32)           # zeros: `/` is NULL there
        self.a_ok = r.random(n_a) >= 0.3
        self.b_ok = r.random(n_b) >= 0.3
        A, B = ("a", self.a_start), ("b", self.b_start)
        self.overlap = ("-", ("least", ("a", self.a_end), ("b", self.b_end)), ("greatest", A, B))      # integer
        self.weighted = ("*", ("b", self.b_score), self.overlap)                                        # float
        self.ratio = ("/", self.overlap, ("b", self.b_div))                                             # float, NULLs
        self.nullable = ("+", ("a", self.a_start, self.a_ok), ("b", self.b_end, self.b_ok))             # NULL columns
        self.only_a = ("abs", ("-", ("a", self.a_score), ("lit", 3)))
        self.only_b = ("-", ("b", self.b_end), ("b", self.b_start))
        self.case = ("if", (">", ("b", self.b_score), ("lit", 0)), self.overlap, ("null",))             # CASE, no ELSE
        self.case_else = ("if", ("isnull", ("b", self.b_start, self.b_ok)), ("lit", 0), self.overlap)
        self.b_score_py = [float(v) for v in self.b_score]
        self.b_end_py = [int(v) if ok else None for v, ok in zip(self.b_end, self.b_ok)]


def run(eng, row_a, row_b, n_a, n_b, aggs, memo=None):
    """``aggs``: ``[(func, tree)]`` or ``[(func, ("col", py_values, array, valid_array_or_None))]``."""
    memo = {} if memo is None else memo
    asked = []
    for func, src in aggs:
        if src[0] == "col":
            _tag, _py, arr, ok = src
            for x in (arr, ok):
                if x is not None and id(x) not in memo:
                    memo[id(x)] = _dev(x.astype(np.uint8) if x.dtype == bool else x)
            asked.append((func, None if arr is None else memo[id(arr)], None if ok is None else memo[id(ok)]))
        else:
            asked.append((func, ("expr", _to_dev(src, memo))))
    return eng.pair_aggregate(_dev(np.asarray(row_a, np.int32)), _dev(np.asarray(row_b, np.int32)), n_a, n_b, asked)


def host(out):
    pairs, res = out
    return pairs.cpu().numpy(), [(v.cpu().numpy(), nn.cpu().numpy()) for v, nn in res]


def _bits(out):
    pairs, res = host(out)
    return [pairs.tobytes()] + [x.tobytes() for pair in res for x in pair]


def _same(a, b) -> bool:
    return a == b or (isinstance(a, float) and isinstance(b, float) and a != a and b != b)


def _is_float_source(src) -> bool:
    if src[0] == "col":
        return src[2] is not None and src[2].dtype.kind == "f"
    return X.E.can_float(src)


def run_and_check(eng, row_a, row_b, n_a, n_b, aggs):
    out = run(eng, row_a, row_b, n_a, n_b, aggs)
    want_pairs, want, inputs = X.pair_expr_aggregate(row_a, row_b, n_a, aggs)
    pairs, res = host(out)
    assert len(res) == len(aggs) and pairs.dtype == np.int64 and pairs.tolist() == want_pairs
    for j, (func, src) in enumerate(aggs):
        flt = _is_float_source(src)
        assert out[1][j][0].dtype == (torch.int64 if func == "COUNT" or (not flt and func != "AVG") else torch.float64)
        vals, nn = (x.tolist() for x in res[j])
        for a in range(n_a):
            xs = inputs[j][a]
            k = sum(x is not None for x in xs)
            what = f"aggregate {j} {func} row {a} of {len(xs)} pairs"
            assert nn[a] == k, what
            w = want[j][a]
            if func == "COUNT":
                assert vals[a] == k, what
            elif w is None:
                assert vals[a] == 0, what
            elif flt and func in ("SUM", "AVG") and w == w and not math.isinf(w):
                bound = k * 2.0**-52 * R.abs_sum(xs)
                bound = bound if func == "SUM" else bound / k + math.ulp(w)
                assert abs(vals[a] - w) <= bound, (what, vals[a], w, bound)
            else:
                assert _same(vals[a], w), (what, vals[a], w)
    return pairs, res


def _random_pairs(r, n, n_a, n_b):
    return r.integers(0, n_a, n), r.integers(0, n_b, n)


# ---------------------------------------------------------------- values
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4096, 4097])
def test_pair_counts_every_function_over_every_kind_of_tree(eng, n):
    r = np.random.default_rng(500 + n)
    n_a, n_b = max(n // 7, 3), max(n // 3, 5)
    t = Tables(n, n_a, n_b)
    row_a, row_b = _random_pairs(r, n, n_a, n_b)
    for tree in (t.overlap, t.weighted, t.ratio, t.case):
        run_and_check(eng, row_a, row_b, n_a, n_b, [(f, tree) for f in FIVE])


def test_regions_across_tiles_fold_steps_and_tile_edges(eng):
    """One call: a region of 257 pairs (crosses a tile), one of 64 x 256 + 257 (crosses a fold step), regions that end
    exactly on a tile edge, A rows without pairs between them, and the last A row."""
    r = np.random.default_rng(21)
    lengths = [TILE, 257, TILE - 1, FOLD * TILE + 257, 2 * TILE - (257 + TILE - 1 + FOLD * TILE + 257) % TILE, TILE, 1, 5]
    rows = [1 + 2 * j for j in range(len(lengths))]
    n_a = rows[-1] + 1                                            # the last A row owns the last region
    n_b = 700
    row_a = np.concatenate([np.full(L, a) for a, L in zip(rows, lengths)])
    ends = np.cumsum(lengths)
    assert ends[0] % TILE == 0 and ends[4] % TILE == 0 and ends[5] % TILE == 0 and rows[-1] == n_a - 1
    row_b = r.integers(0, n_b, len(row_a))
    order = r.permutation(len(row_a))
    t = Tables(22, n_a, n_b)
    pairs, res = run_and_check(eng, row_a[order], row_b[order], n_a, n_b,
                               [("SUM", t.overlap), ("SUM", t.weighted), ("MIN", t.ratio), ("COUNT", t.case),
                                ("AVG", t.overlap), ("MAX", t.only_a)])
    want = np.zeros(n_a, np.int64)
    want[rows] = lengths
    assert pairs.tolist() == want.tolist()
    for vals, nn in res:
        assert not nn[want == 0].any() and not vals[want == 0].any()


def test_one_row_owns_all_pairs(eng):
    r = np.random.default_rng(23)
    n, n_a, n_b = 3 * TILE + 11, 5, 300
    t = Tables(24, n_a, n_b)
    pairs, _res = run_and_check(eng, np.full(n, 2), r.integers(0, n_b, n), n_a, n_b,
                                [("SUM", t.overlap), ("AVG", t.weighted), ("MAX", t.ratio)])
    assert pairs.tolist() == [0, 0, n, 0, 0]


@pytest.mark.parametrize("n_a,n_b", [(1, 1), (256, 257), (257, 256), (65536, 65537), (65537, 65536), (1, 65537)])
def test_table_sizes_at_the_digit_boundaries_with_the_top_ids(eng, n_a, n_b):
    r = np.random.default_rng(n_a + 3 * n_b)
    n = 1500
    row_a, row_b = _random_pairs(r, n, n_a, n_b)
    row_a[:4] = [n_a - 1, n_a - 1, 0, max(n_a - 2, 0)]
    row_b[:4] = [n_b - 1, 0, n_b - 1, n_b - 1]
    t = Tables(25, n_a, n_b)
    out = run(eng, row_a, row_b, n_a, n_b, [("SUM", t.overlap), ("SUM", t.weighted), ("COUNT", t.ratio)])
    pairs, res = host(out)
    # the reference over the rows that have pairs (65,537 Python rows of nothing would only cost time)
    used = np.unique(row_a)
    dense = np.searchsorted(used, row_a)
    want_pairs, want, inputs = X.pair_expr_aggregate(dense, row_b, len(used), [
        ("SUM", _reindex_a(t.overlap, used)), ("SUM", _reindex_a(t.weighted, used)), ("COUNT", _reindex_a(t.ratio, used))])
    assert pairs[used].tolist() == want_pairs and int(pairs.sum()) == n
    assert res[0][0][used].tolist() == [w or 0 for w in want[0]]
    for a, (w, xs) in enumerate(zip(want[1], inputs[1])):
        assert abs(res[1][0][used[a]] - (w or 0.0)) <= len(xs) * 2.0**-52 * R.abs_sum(xs)
    assert res[2][0][used].tolist() == want[2]
    mask = np.ones(n_a, bool)
    mask[used] = False
    assert all(not v[mask].any() and not nn[mask].any() for v, nn in res)


def _reindex_a(tree, used):
    """The tree with every A column cut to the rows ``used`` (dense A ids)."""
    if tree[0] == "a":
        return ("a",) + tuple(None if x is None else x[used] for x in tree[1:])
    if tree[0] in ("b", "lit", "null"):
        return tree
    return (tree[0],) + tuple(_reindex_a(c, used) for c in tree[1:])


def test_null_columns_a_row_of_nulls_only_and_one_sided_trees(eng):
    r = np.random.default_rng(26)
    n_a, n_b = 50, 400
    row_a, row_b = _random_pairs(r, 3000, n_a, n_b)
    row_a[row_a == 18] = 19                              # row 18 has no pair at all
    t = Tables(27, n_a, n_b)
    t.a_ok[17] = False                                   # every value of row 17 is NULL: a.start is
    t.b_div[row_b[row_a == 16]] = 0                      # ... and of row 16 under `/`
    pairs, res = run_and_check(eng, row_a, row_b, n_a, n_b,
                               [(f, t.nullable) for f in FIVE] + [("SUM", t.ratio), ("MIN", t.only_a), ("MAX", t.only_b)])
    assert pairs[17] > 0 and pairs[16] > 0 and pairs[18] == 0
    for vals, nn in res[:5]:
        assert nn[17] == 0 and vals[17] == 0 and nn[18] == 0 and vals[18] == 0
    assert res[5][1][16] == 0 and res[5][0][16] == 0 and res[6][1][17] == pairs[17]


def test_eight_aggregates_mixing_columns_and_expressions(eng):
    r = np.random.default_rng(28)
    n, n_a, n_b = 5000, 211, 777
    row_a, row_b = _random_pairs(r, n, n_a, n_b)
    t = Tables(29, n_a, n_b)
    score = ("col", t.b_score_py, t.b_score, None)
    end = ("col", t.b_end_py, t.b_end, t.b_ok)
    name = ("col", [1 if ok else None for ok in t.b_ok], None, t.b_ok)
    run_and_check(eng, row_a, row_b, n_a, n_b,
                  [("SUM", t.overlap), ("AVG", score), ("AVG", t.overlap), ("MAX", end), ("COUNT", name),
                   ("SUM", t.weighted), ("MIN", t.case_else), ("COUNT", t.ratio)])
    with pytest.raises(ValueError, match="at most 8"):
        run(eng, row_a, row_b, n_a, n_b, [("MIN", t.overlap)] * 9)


def _chain(leaf, n_nodes):
    """A tree of exactly ``n_nodes`` nodes: leaf + 0 + 0 + ... (each `+ 0` adds two)."""
    assert n_nodes % 2 == 1
    tree = leaf
    for _ in range(n_nodes // 2):
        tree = ("+", tree, ("lit", 0))
    return tree


def test_the_256_node_limit_and_one_past_it(eng):
    r = np.random.default_rng(30)
    n_a, n_b = 9, 40
    row_a, row_b = _random_pairs(r, 600, n_a, n_b)
    t = Tables(31, n_a, n_b)
    # four chains of 9 stack-shallow nodes would not reach the limit: 255 + 1 nodes in two programs do
    long, one = _chain(("b", t.b_start), 255), ("a", t.a_start)
    pairs, res = run_and_check(eng, row_a, row_b, n_a, n_b, [("SUM", long), ("MAX", one)])
    assert int(pairs.sum()) == 600
    with pytest.raises(ValueError, match="256 expression nodes"):
        run(eng, row_a, row_b, n_a, n_b, [("SUM", long), ("MAX", ("neg", one))])


# ---------------------------------------------------------------- determinism
def test_order_invariance_and_repeat_runs_are_bit_identical(eng):
    r = np.random.default_rng(32)
    n, n_a, n_b = 12293, 97, 4001
    row_a, row_b = _random_pairs(r, n, n_a, n_b)
    t = Tables(33, n_a, n_b)
    # values of very different magnitude: a float sum taken in another order would round differently
    wild = (r.normal(0, 1, n_b) * 10.0 ** r.integers(-8, 9, n_b)).astype(np.float64)
    tree = ("*", ("b", wild), ("+", ("a", t.a_score), ("lit", 0.5)))
    aggs = [("SUM", tree), ("AVG", tree), ("MIN", t.ratio), ("SUM", t.overlap), ("COUNT", t.case),
            ("SUM", ("col", t.b_score_py, t.b_score, None))]
    memo = {}
    first = _bits(run(eng, row_a, row_b, n_a, n_b, aggs, memo))
    assert _bits(run(eng, row_a, row_b, n_a, n_b, aggs, memo)) == first            # the same call twice
    assert _bits(run(eng, row_a[::-1], row_b[::-1], n_a, n_b, aggs, memo)) == first
    for seed in (11, 12, 13):
        p = np.random.default_rng(seed).permutation(n)
        assert _bits(run(eng, row_a[p], row_b[p], n_a, n_b, aggs, memo)) == first, seed


SORT_FORMS = {
    "default": {},
    "three-stage": {"GIQL_HIP_LOCAL_MIN_ROWS": "1"},
    "narrow": {"GIQL_HIP_LOCAL_MIN_ROWS": "1", "GIQL_HIP_LOCAL_BITS": "13"},
    "classic": {"GIQL_HIP_SORT": "classic"},
    "os-variant-3": {"GIQL_HIP_OS_VARIANT": "3"},
    "no-local": {"GIQL_HIP_NO_LOCAL_SORT": "1"},
}


def test_every_sort_form_of_the_context_gives_the_same_bits(eng, monkeypatch):
    from giql_amd.engine import HipEngine

    r = np.random.default_rng(34)
    n, n_a, n_b = 9000, 300, 70000
    row_a, row_b = _random_pairs(r, n, n_a, n_b)
    t = Tables(35, n_a, n_b)
    aggs = [("SUM", t.weighted), ("AVG", t.ratio), ("MIN", t.overlap), ("COUNT", t.nullable)]
    memo = {}
    first = _bits(run(eng, row_a, row_b, n_a, n_b, aggs, memo))
    for name, env in SORT_FORMS.items():
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        e = HipEngine(0)
        try:
            assert _bits(run(e, row_a, row_b, n_a, n_b, aggs, memo)) == first, name
        finally:
            e.close()
            for k in env:
                monkeypatch.delenv(k)


# ---------------------------------------------------------------- the raw entry point
class Raw:
    """A raw ``giql_hip_pair_expr_agg_dev`` call over 3 pairs of a 5 x 9 join with one program, ``b.v + 1``."""

    def __init__(self, eng):
        from giql_amd import _lib

        self.eng, self.lib = eng, _lib
        self.n_a, self.n_b = 5, 9
        self.ra, self.rb = _dev(np.array([0, 1, 4], np.int32)), _dev(np.array([8, 0, 3], np.int32))
        self.data = _dev(np.arange(self.n_b, dtype=np.int64))
        self.fdata = _dev(np.arange(self.n_b, dtype=np.float64))
        self.out = torch.zeros(self.n_a, dtype=torch.int64, device="cuda:0")
        self.nn = torch.zeros(self.n_a, dtype=torch.int64, device="cuda:0")
        self.pairs = torch.zeros(self.n_a, dtype=torch.int64, device="cuda:0")

    def nodes(self, flt=False):
        c = (self.lib.COperand * 3)()
        c[0].side, c[0].type = self.lib.SIDE_B, self.lib.T_F64 if flt else self.lib.T_I64
        c[0].data = (self.fdata if flt else self.data).data_ptr()
        c[1].side, c[1].lit_i = self.lib.SIDE_LIT, 1
        c[2].side = 16  # GIQL_X_ADD
        return c

    def agg(self, func=1, typ=None, first=0, count=3, o=True, d=False):
        c = (self.lib.CPairExprAgg * 9)()
        for k in range(9):
            c[k].func, c[k].type = func, self.lib.T_I64 if typ is None else typ
            c[k].first, c[k].count = first, count
            c[k].data = self.data.data_ptr() if d else None
            c[k].out, c[k].out_nn = (self.out.data_ptr() if o else None), self.nn.data_ptr()
        return c

    def call(self, nodes, n_nodes, aggs, n_aggs, n_pairs=3, ra=True, pairs=True, n_a=None):
        return self.eng._L.giql_hip_pair_expr_agg_dev(
            self.eng._h, self.ra.data_ptr() if ra else None, self.rb.data_ptr(), n_pairs,
            self.n_a if n_a is None else n_a, self.n_b, nodes, n_nodes, aggs, n_aggs,
            self.pairs.data_ptr() if pairs else None, self.eng._stream())


def _hold_a_plan(eng):
    from giql_amd.engine import DeviceSide

    s = DeviceSide.from_numpy(np.zeros(4, np.int32), np.arange(4, dtype=np.int32) * 10,
                              np.arange(4, dtype=np.int32) * 10 + 15, device="cuda:0")
    assert eng.inner_plan(s, s, 1) > 0


def _plan_is_gone(eng):
    from giql_amd import _lib

    a = torch.empty(4, dtype=torch.int32, device="cuda:0")
    assert eng._L.giql_hip_inner_fill_dev(eng._h, a.data_ptr(), a.data_ptr(), 4, eng._stream()) == _lib.GIQL_ERR_STATE


def test_the_raw_call_and_its_argument_errors(eng):
    w = Raw(eng)
    L = w.lib
    _hold_a_plan(eng)
    assert w.call(w.nodes(), 3, w.agg(), 1) == L.GIQL_OK
    assert w.out.tolist() == [9, 1, 0, 0, 4] and w.nn.tolist() == [1, 1, 0, 0, 1] and w.pairs.tolist() == [1, 1, 0, 0, 1]
    _plan_is_gone(eng)                                       # a held plan is dropped by the call
    bad = [
        dict(nodes=w.nodes(flt=True), n_nodes=3, aggs=w.agg(), n_aggs=1),           # a float program typed I64
        dict(nodes=w.nodes(), n_nodes=3, aggs=w.agg(), n_aggs=9),                   # n_aggs outside 0..8
        dict(nodes=w.nodes(), n_nodes=3, aggs=w.agg(), n_aggs=-1),
        dict(nodes=w.nodes(), n_nodes=257, aggs=w.agg(), n_aggs=1),                 # n_nodes outside 0..256
        dict(nodes=None, n_nodes=3, aggs=w.agg(), n_aggs=1),                        # NULL nodes
        dict(nodes=w.nodes(), n_nodes=3, aggs=w.agg(count=4), n_aggs=1),            # a range outside the nodes
        dict(nodes=w.nodes(), n_nodes=3, aggs=w.agg(count=2), n_aggs=1),            # malformed: two values left
        dict(nodes=w.nodes(), n_nodes=3, aggs=w.agg(typ=L.T_I32), n_aggs=1),        # a program typed int32
        dict(nodes=w.nodes(), n_nodes=3, aggs=w.agg(o=False), n_aggs=1),            # NULL out
        dict(nodes=w.nodes(), n_nodes=3, aggs=w.agg(func=4), n_aggs=1),             # unknown function
        dict(nodes=w.nodes(), n_nodes=3, aggs=w.agg(count=0), n_aggs=1),            # a column source, NULL data, SUM
        dict(nodes=w.nodes(), n_nodes=3, aggs=None, n_aggs=1),                      # NULL aggs
        dict(nodes=w.nodes(), n_nodes=3, aggs=w.agg(), n_aggs=1, ra=False),         # NULL row_a
        dict(nodes=w.nodes(), n_nodes=3, aggs=w.agg(), n_aggs=1, pairs=False),      # NULL pairs_out
        dict(nodes=w.nodes(), n_nodes=3, aggs=w.agg(), n_aggs=1, n_pairs=1 << 31),  # too many pairs
    ]
    for kw in bad:
        _hold_a_plan(eng)
        w.out.fill_(77)
        assert w.call(**kw) == L.GIQL_ERR_INVALID, {k: v for k, v in kw.items() if k not in ("nodes", "aggs")}
        _plan_is_gone(eng)
    assert b"float" in (w.call(w.nodes(flt=True), 3, w.agg(), 1), eng._L.giql_hip_last_error())[1]
    # a float program under GIQL_T_F64, and the conventions of no pairs / no left rows
    assert w.call(w.nodes(flt=True), 3, w.agg(typ=L.T_F64), 1) == L.GIQL_OK
    assert w.out.view(torch.float64).tolist() == [9.0, 1.0, 0.0, 0.0, 4.0]
    w.out.fill_(77), w.pairs.fill_(77)
    assert w.call(w.nodes(), 3, w.agg(), 1, n_pairs=0) == L.GIQL_OK and not w.out.any() and not w.pairs.any()
    w.out.fill_(77), w.pairs.fill_(77)
    assert w.call(w.nodes(), 3, w.agg(), 1, n_pairs=0, n_a=0) == L.GIQL_OK
    assert w.out.tolist() == [77] * 5 and w.pairs.tolist() == [77] * 5


def test_a_call_without_an_expression_gives_the_bits_of_the_column_entry_point(eng):
    """The new entry point with column sources alone against ``giql_hip_pair_agg_dev`` on the same input."""
    from giql_amd import _lib

    r = np.random.default_rng(36)
    n, n_a, n_b = 9001, 123, 5000
    row_a, row_b = (_dev(x.astype(np.int32)) for x in _random_pairs(r, n, n_a, n_b))
    vals = _dev((r.normal(0, 1, n_b) * 10.0 ** r.integers(-8, 9, n_b)).astype(np.float64))
    ints = _dev(r.integers(-1000, 1000, n_b).astype(np.int32))
    ok = _dev((r.random(n_b) >= 0.3).astype(np.uint8))
    spec = [(1, _lib.T_F64, vals, ok), (2, _lib.T_F64, vals, None), (3, _lib.T_I32, ints, ok), (0, _lib.T_I32, None, ok)]
    got = []
    for cls in (_lib.CAgg, _lib.CPairExprAgg):
        c = (cls * len(spec))()
        outs = [(torch.empty(n_a, dtype=torch.int64, device="cuda:0"), torch.empty(n_a, dtype=torch.int64, device="cuda:0"))
                for _ in spec]
        for k, (func, typ, data, valid) in enumerate(spec):
            c[k].func, c[k].type = func, typ
            c[k].data = None if data is None else data.data_ptr()
            c[k].valid = None if valid is None else valid.data_ptr()
            c[k].out, c[k].out_nn = outs[k][0].data_ptr(), outs[k][1].data_ptr()
        pairs = torch.empty(n_a, dtype=torch.int64, device="cuda:0")
        if cls is _lib.CAgg:
            rc = eng._L.giql_hip_pair_agg_dev(eng._h, row_a.data_ptr(), row_b.data_ptr(), n, n_a, n_b, c, len(spec),
                                              pairs.data_ptr(), eng._stream())
        else:
            rc = eng._L.giql_hip_pair_expr_agg_dev(eng._h, row_a.data_ptr(), row_b.data_ptr(), n, n_a, n_b, None, 0, c,
                                                   len(spec), pairs.data_ptr(), eng._stream())
        assert rc == _lib.GIQL_OK
        got.append([pairs.cpu().numpy().tobytes()] + [x.cpu().numpy().tobytes() for pair in outs for x in pair])
    assert got[0] == got[1]


@pytest.mark.parametrize("where,value", [("a", 5), ("a", -1), ("b", 9), ("b", -1), ("a", 2**31 - 1), ("b", -2**31)])
def test_an_id_outside_its_table_is_an_argument_error(eng, where, value):
    """One bad id among 257 pairs: found by the load pass before any program reads through it."""
    from giql_amd._lib import GIQL_ERR_INVALID, GiqlHipError

    r = np.random.default_rng(37)
    n_a, n_b = 5, 9
    row_a, row_b = _random_pairs(r, 257, n_a, n_b)
    (row_a if where == "a" else row_b)[200] = value
    t = Tables(38, n_a, n_b)
    _hold_a_plan(eng)
    with pytest.raises(GiqlHipError) as err:
        run(eng, row_a, row_b, n_a, n_b, [("SUM", t.weighted), ("MIN", t.overlap)])
    assert err.value.code == GIQL_ERR_INVALID and "outside" in str(err.value)
    _plan_is_gone(eng)


def test_engine_argument_errors(eng):
    t = Tables(39, 5, 9)
    with pytest.raises(ValueError, match="one value per row of its table"):
        run(eng, [0], [0], 5, 9, [("SUM", ("+", ("a", t.b_start), ("lit", 1)))])      # a B-sized column as side a
    with pytest.raises(ValueError, match="aggregate function"):
        run(eng, [0], [0], 5, 9, [("MEDIAN", t.overlap)])
    with pytest.raises(ValueError, match="expression operator"):
        run(eng, [0], [0], 5, 9, [("SUM", ("%", ("a", t.a_start), ("lit", 2)))])


def test_the_call_runs_on_a_side_stream_behind_pending_work(eng):
    """The stale / fresh protocol of tests/_stream_harness.py for this call: the device buffers are rewritten from
    STALE to FRESH on a side stream behind a delay; the call, issued on that stream, must see FRESH, and the
    buffers go back to STALE behind it."""
    r = np.random.default_rng(40)
    n, n_a, n_b = 5000, 40, 600
    sets, want = {}, {}
    for name in ("stale", "fresh"):
        ra, rb = _random_pairs(r, n, n_a, n_b)
        s = {"row_a": ra.astype(np.int32), "row_b": rb.astype(np.int32),
             "a": r.integers(0, 1000, n_a).astype(np.int64), "b": r.integers(0, 1000, n_b).astype(np.int64)}
        tree = ("abs", ("-", ("a", s["a"]), ("b", s["b"])))
        want[name] = X.pair_expr_aggregate(ra, rb, n_a, [("SUM", tree), ("MAX", tree)])
        sets[name] = s
    assert want["stale"][1] != want["fresh"][1]
    bufs = {k: _dev(v) for k, v in sets["stale"].items()}
    fresh = {k: _dev(v) for k, v in sets["fresh"].items()}
    stale = {k: _dev(v) for k, v in sets["stale"].items()}
    tree = ("expr", ("abs", ("-", ("a", bufs["a"]), ("b", bufs["b"]))))
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)                        # pending work the call has to queue behind
        for k in bufs:
            bufs[k].copy_(fresh[k], non_blocking=True)
        out = eng.pair_aggregate(bufs["row_a"], bufs["row_b"], n_a, n_b, [("SUM", tree), ("MAX", tree)])
        for k in bufs:
            bufs[k].copy_(stale[k], non_blocking=True)
        pairs, res = host(out)
    side.synchronize()
    assert pairs.tolist() == want["fresh"][0]
    assert res[0][0].tolist() == [w or 0 for w in want["fresh"][1][0]]
    assert res[1][0].tolist() == [w or 0 for w in want["fresh"][1][1]]
    assert all(torch.equal(bufs[k], stale[k]) for k in bufs)
