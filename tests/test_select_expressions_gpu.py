"""Computed SELECT-list columns on the GPU: ``HipEngine.eval_exprs`` / ``giql_hip_eval_expr_dev`` against the
plain-Python reference of ``_expr_ref`` bit for bit (every step is one correctly rounded operation: there is no
tolerance), the limits of the C ABI, and the ``-wo`` / ``-wao`` recipes through ``transpile(...,
select_expressions=True)`` + ``execute()``."""
import ctypes
import json
import os

import numpy as np
import pytest

import _expr_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


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
    """Trees over numpy arrays -> the same trees over device tensors (one upload per array); ``rows`` re-addresses a
    side by the candidate index: its columns are gathered by the ids the call then leaves out."""

    def __init__(self, rows=None):
        self.cache, self.rows = {}, rows or {}

    def tensor(self, side, x):
        key = (side, id(x))
        if key not in self.cache:
            y = x[self.rows[side]] if side in self.rows else x
            self.cache[key] = (x, _torch().from_numpy(np.ascontiguousarray(y)).cuda())
        return self.cache[key][1]

    def tree(self, t):
        if t[0] in ("a", "b"):
            return (t[0], *[self.tensor(t[0], x) for x in t[1:]])
        if t[0] in ("lit", "null"):
            return t
        return (t[0], *[self.tree(c) for c in t[1:]])


def _same(got, want, what):
    """One output against the reference: integers exactly, floats by bit pattern (NaN by isnan), validity exactly,
    ``valid`` None exactly when the reference has no NULL."""
    (gv, gok), (wv, wok) = got, want
    gv = gv.cpu().numpy()
    assert gv.dtype == wv.dtype, (what, gv.dtype, wv.dtype)
    n_null = int((wok == 0).sum())
    if n_null == 0:
        assert gok is None, f"{what}: a validity tensor for an output without a NULL"
    else:
        assert gok is not None, f"{what}: {n_null} NULLs expected, none reported"
        bad = np.nonzero(gok.cpu().numpy() != wok)[0]
        assert not bad.size, f"{what}: validity differs at {bad[:5].tolist()} of {len(wok)}"
    if wv.dtype == np.float64:
        bad = np.nonzero(R.bits(gv) != R.bits(wv))[0]
    else:
        bad = np.nonzero(gv != wv)[0]
    assert not bad.size, f"{what}: {bad.size} values differ, first at {bad[:5].tolist()}: {gv[bad[:5]]} != {wv[bad[:5]]}"


def _eval(eng, trees, ia, ib, n_a, n_b, mode=0):
    """``eng.eval_exprs``; mode bit 0 / 1 = leave idx_a / idx_b out ("the candidate index": only for ids >= 0)."""
    torch = _torch()
    n = len(ia)
    rows = {s: x.astype(np.int64) for s, x, bit in (("a", ia, 1), ("b", ib, 2)) if mode & bit}
    dev = _Dev(rows)
    ida = None if mode & 1 else torch.from_numpy(ia).cuda()
    idb = None if mode & 2 else torch.from_numpy(ib).cuda()
    return eng.eval_exprs([dev.tree(t) for t in trees], idx_a=ida, idx_b=idb, n=n, n_rows_a=n if mode & 1 else n_a,
                          n_rows_b=n if mode & 2 else n_b)


# ---- the generated differential test: sizes at the wave, tile and multi-block edges, 8 programs per call
@pytest.mark.parametrize("k", range(len(R.GPU_CASES)), ids=[f"seed{s}-n{n}" for s, n in R.GPU_CASES])
def test_generated_expressions_match_the_reference(eng, k):
    seed, n = R.GPU_CASES[k]
    d, ia, ib, expected = R.draw(seed, n)
    got = _eval(eng, d.trees, ia, ib, d.N_A, d.N_B)
    assert len(got) == len(d.trees) == 8
    for j, (g, w) in enumerate(zip(got, expected)):
        _same(g, w, f"seed {seed} n {n} tree {j}")
    print(f"seed {seed} n {n}: nodes {[R.count_nodes(t) for t in d.trees]}, NULLs {[int((w[1] == 0).sum()) for w in expected]}")


@pytest.mark.parametrize("n_trees", [1, 2, 8, 9])
def test_one_two_eight_programs_in_one_call_and_nine_in_two(eng, n_trees, monkeypatch):
    d, ia, ib, expected = R.draw(22, 2049, n_trees=n_trees)
    assert sum(R.count_nodes(t) for t in d.trees[:8]) <= 256        # (so 8 programs do share one call)
    calls = []
    real = eng._L.giql_hip_eval_expr_dev

    class Spy:
        def giql_hip_eval_expr_dev(self, *args):
            calls.append(int(args[4]))
            return real(*args)

        def __getattr__(self, name):
            return getattr(eng._L, name)

    monkeypatch.setattr(eng, "_L", Spy())
    got = _eval(eng, d.trees, ia, ib, d.N_A, d.N_B)
    assert calls == ([n_trees] if n_trees <= 8 else [8, 1])
    for j, (g, w) in enumerate(zip(got, expected)):
        _same(g, w, f"{n_trees} trees, tree {j}")


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_missing_id_arrays_mean_the_candidate_index(eng, mode):
    d, ia, ib, _ = R.draw(25, 2049)
    # a side without ids cannot name the NULL row: those candidates keep valid ids on that side
    ia = np.where(ia < 0, 0, ia).astype(np.int32) if mode & 1 else ia
    ib = np.where(ib < 0, 0, ib).astype(np.int32) if mode & 2 else ib
    expected = d.expected(ia, ib)
    for j, (g, w) in enumerate(zip(_eval(eng, d.trees, ia, ib, d.N_A, d.N_B, mode=mode), expected)):
        _same(g, w, f"mode {mode} tree {j}")


def test_null_rows_on_either_side_and_on_both(eng):
    """-1 ids mixed in among valid ones: every column of that side is NULL, whatever its validity pointer."""
    torch = _torch()
    n_a, n_b = 5, 4
    va = np.arange(10, 10 + n_a, dtype=np.int32)
    vb = np.array([1.5, 2.5, 3.5, 4.5])
    okb = np.array([1, 0, 1, 1], np.uint8)
    A, B = ("a", va), ("b", vb, okb)
    trees = [("+", A, ("lit", 1)), ("*", B, ("lit", 2.0)), ("+", A, B), ("isnull", B), ("isnull", A),
             ("if", ("isnull", B), ("lit", 0), ("-", A, ("lit", 10))), ("least", A, B), ("if", ("isnull", A), ("null",), A)]
    ia = np.array([0, -1, 2, -1, 4, 3, -1], np.int32)
    ib = np.array([0, 1, -1, -1, 1, 3, 2], np.int32)
    got = _eval(eng, trees, ia, ib, n_a, n_b)
    for j, (g, t) in enumerate(zip(got, trees)):
        _same(g, R.evaluate(t, ia, ib), f"tree {j}")
    # spelt out for the -wao shape: 0 where the right side is NULL (a padded row, or a NULL value), the value
    # elsewhere -- NULL on the last candidate, whose right side is there and whose LEFT side is the NULL row
    v, ok = got[5]
    assert ok.cpu().tolist() == [1, 1, 1, 1, 1, 1, 0] and v.cpu().tolist() == [0, 0, 0, 0, 0, 3, 0]
    v, ok = got[0]
    assert ok.cpu().tolist() == [1, 0, 1, 0, 1, 1, 0] and v.cpu().tolist() == [11, 0, 13, 0, 15, 14, 0]
    # an empty right table: every id on it is the NULL row
    empty = ("b", np.zeros(0, np.int64))
    dev = _Dev()
    v, ok = eng.eval_exprs([dev.tree(("if", ("isnull", empty), ("lit", 7), empty))], idx_a=torch.from_numpy(ia[:3] * 0).cuda(),
                           idx_b=torch.full((3,), -1, dtype=torch.int32, device="cuda"), n_rows_a=n_a, n_rows_b=0)[0]
    assert ok is None and v.cpu().tolist() == [7, 7, 7]


def test_a_256_node_program_and_a_12_deep_one(eng):
    d, ia, ib, expected = R.draw(24, 2049)          # 24 % 3 == 0: tree 1 holds 256 nodes; 24 % 12 == 0 -> depth 1
    assert R.count_nodes(d.trees[1]) == 256
    d12, ia12, ib12, expected12 = R.draw(23, 2049)   # 23 % 12 == 11 -> the first tree keeps 12 values live
    assert R.live_values(d12.trees[0]) == 12
    _same(_eval(eng, d.trees[1:2], ia, ib, d.N_A, d.N_B)[0], expected[1], "256 nodes")
    _same(_eval(eng, d12.trees[:1], ia12, ib12, d12.N_A, d12.N_B)[0], expected12[0], "12 deep")


# ---- the C ABI through ctypes
def _abi(eng):
    from giql_amd import _lib

    torch = _torch()
    L, n = eng._L, 8
    col = torch.arange(n, dtype=torch.int32, device="cuda")
    fcol = torch.arange(n, dtype=torch.float64, device="cuda")

    def lit(v):
        o = _lib.COperand()
        o.side, o.lit_i = _lib.SIDE_LIT, v
        return o

    def node(kind):
        o = _lib.COperand()
        o.side = kind
        return o

    def column(t=col, typ=_lib.T_I32, side=_lib.SIDE_A):
        o = _lib.COperand()
        o.side, o.type, o.data = side, typ, t.data_ptr()
        return o

    def call(nodes, outs, n_outs=None, n_nodes=None, idx_a=None, n_rows_a=n, n_cand=n, want_nulls=True):
        """outs: [(first, count, type, data tensor | None, valid tensor | None)]"""
        c_nodes = (_lib.COperand * max(len(nodes), 1))(*nodes)
        c_outs = (_lib.CExprOut * max(len(outs), 1))()
        for j, (first, count, typ, data, valid) in enumerate(outs):
            c_outs[j].first, c_outs[j].count, c_outs[j].type = first, count, typ
            c_outs[j].data = data.data_ptr() if data is not None else None
            c_outs[j].valid = valid.data_ptr() if valid is not None else None
        nulls = (ctypes.c_int64 * 9)(*([-5] * 9))
        rc = L.giql_hip_eval_expr_dev(eng._h, c_nodes, len(nodes) if n_nodes is None else n_nodes, c_outs,
                                      len(outs) if n_outs is None else n_outs,
                                      idx_a.data_ptr() if idx_a is not None else None, n_rows_a, None, 0, n_cand,
                                      nulls if want_nulls else None, None)
        return rc, (L.giql_hip_last_error() or b"").decode(), list(nulls)

    return _lib, torch, n, col, fcol, lit, node, column, call


def test_c_abi_refuses_what_it_must_and_still_answers(eng):
    _lib, torch, n, col, fcol, lit, node, column, call = _abi(eng)
    ADD, DIV = eng._XOPS["+"], eng._XOPS["/"]
    out = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    ok = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    I64, F64, I32 = _lib.T_I64, _lib.T_F64, _lib.T_I32
    deep13 = [lit(1)] * 13 + [node(ADD)] * 12
    big = torch.tensor([0, 1, n, 2], dtype=torch.int32, device="cuda")
    refusals = [
        ("257 nodes", [lit(1)] * 257, [(0, 1, I64, out, ok)], {}, "at most 256 expression nodes"),
        ("depth 13", deep13, [(0, 25, I64, out, ok)], {}, "output 0 program: expression deeper than 12"),
        ("IF on two values", [lit(1), lit(2), node(_lib.X_IF)], [(0, 3, I64, out, ok)], {}, "output 0 program: malformed expression"),
        ("an unknown node kind", [lit(1), node(99)], [(0, 2, I64, out, ok)], {}, "output 0 program: expression node kind 99"),
        ("n_outs 0", [lit(1)], [(0, 1, I64, out, ok)], {"n_outs": 0}, "n_outs = 0 outside [1, 8]"),
        ("n_outs 9", [lit(1)], [(0, 1, I64, out, ok)] * 9, {}, "n_outs = 9 outside [1, 8]"),
        ("a NULL data", [lit(1)], [(0, 1, I64, out, ok), (0, 1, I64, None, ok)], {}, "output 1: data is NULL"),
        ("type GIQL_T_I32", [lit(1)], [(0, 1, I32, out, ok)], {}, "output 0: type 0"),
        ("an I64 output for a program with /", [column(), lit(2), node(DIV)], [(0, 1, I64, out, ok), (0, 3, I64, out, ok)], {},
         "output 1: the program can yield a float"),
        ("an I64 output for a float column", [column(fcol, _lib.T_F64)], [(0, 1, I64, out, ok)], {}, "output 0: the program can yield a float"),
        ("a program past the nodes", [lit(1)], [(0, 2, I64, out, ok)], {}, "output 0 program: expression nodes [0, 2) outside the 1 given"),
    ]
    for what, nodes, outs, kw, message in refusals:
        rc, err, _ = call(nodes, outs, **kw)
        assert rc == _lib.GIQL_ERR_INVALID, what
        assert message in err, (what, err)
    assert bool((out == -1).all()) and bool((ok == 9).all())         # nothing was launched, nothing written
    # an id >= n_rows: GIQL_ERR_INVALID from the device, and a usable context afterwards
    rc, err, _ = call([column()], [(0, 1, I64, out, ok)], idx_a=big, n_cand=4)
    assert rc == _lib.GIQL_ERR_INVALID and "row id" in err, err
    # n == 0: GIQL_OK, nothing launched, the counts zeroed
    out.fill_(-1)
    rc, err, nulls = call([column()], [(0, 1, I64, None, None)], n_cand=0)
    assert rc == _lib.GIQL_OK and nulls[0] == 0 and bool((out == -1).all()), err
    # a valid call: col + 1 and IF(col > 3, NULL, col / 2) in one pass, with and without a validity pointer
    fout = torch.full((n,), -1.0, dtype=torch.float64, device="cuda")
    GT = eng._XOPS[">"]
    nodes = [column(), lit(1), node(ADD),
             column(), lit(3), node(GT), node(_lib.X_NULL), column(), lit(2), node(DIV), node(_lib.X_IF)]
    rc, err, nulls = call(nodes, [(0, 3, I64, out, None), (3, 8, F64, fout, ok)])
    assert rc == _lib.GIQL_OK, err
    assert nulls[:3] == [0, 4, -5]
    assert out.cpu().tolist() == [1, 2, 3, 4, 5, 6, 7, 8]
    assert ok.cpu().tolist() == [1, 1, 1, 1, 0, 0, 0, 0] and fout.cpu().tolist() == [0.0, 0.5, 1.0, 1.5, 0.0, 0.0, 0.0, 0.0]
    # an F64 output converts an integer value; n_null may be NULL
    rc, err, _ = call([column(), lit(1), node(ADD)], [(0, 3, F64, fout, None)], want_nulls=False)
    assert rc == _lib.GIQL_OK and fout.cpu().tolist() == [float(i + 1) for i in range(n)], err


def test_the_call_drops_a_plan_held_on_the_context(eng):
    from giql_amd.engine import DeviceSide

    _lib, torch, n, col, fcol, lit, node, column, call = _abi(eng)
    c = np.zeros(6, np.int32)
    s = np.arange(6, dtype=np.int32) * 10
    a = DeviceSide.from_numpy(c, s, s + 15, device="cuda:0")
    b = DeviceSide.from_numpy(c, s + 5, s + 12, device="cuda:0")
    n_pairs = eng.inner_plan(a, b, 1)
    assert n_pairs > 0
    out = torch.empty(n, dtype=torch.int64, device="cuda")
    rc, err, _ = call([column()], [(0, 1, _lib.T_I64, out, None)])
    assert rc == _lib.GIQL_OK, err
    ra = torch.empty(n_pairs, dtype=torch.int32, device="cuda")
    rb = torch.empty(n_pairs, dtype=torch.int32, device="cuda")
    rc = eng._L.giql_hip_inner_fill_dev(eng._h, ra.data_ptr(), rb.data_ptr(), n_pairs, None)
    assert rc == _lib.GIQL_ERR_STATE
    # ... and the context goes on: plan and fill again
    assert eng.inner_plan(a, b, 1) == n_pairs
    eng.inner_fill(ra, rb)


def test_select_takes_if_and_null_in_a_boolean_program_and_still_rejects_negative_ids(eng):
    from giql_amd._lib import GiqlHipError

    torch = _torch()
    va = np.array([1, 5, 9, 3, 7], np.int32)
    oka = np.array([1, 1, 0, 1, 1], np.uint8)
    A = ("a", va, oka)
    # keep where CASE WHEN a > 4 THEN a ELSE NULL END < 8  (NULL: not kept)
    tree = ("<", ("if", (">", A, ("lit", 4)), A, ("null",)), ("lit", 8))
    dev = _Dev()
    ids = torch.arange(5, dtype=torch.int32, device="cuda")
    kept = eng.select([(("expr", dev.tree(tree)), "istrue", ("lit", 0))], idx_a=ids, n_rows_a=5, want=("a",))[0]
    want = [i for i, v in enumerate(R.values(tree, list(range(5)), list(range(5)))) if v is True]
    assert kept.cpu().tolist() == want == [1, 4]
    neg = torch.tensor([0, -1, 2], dtype=torch.int32, device="cuda")
    with pytest.raises(GiqlHipError) as exc:
        eng.select([(dev.tree(A), ">", ("lit", 0))], idx_a=neg, n_rows_a=5, want=("a",))
    assert exc.value.code == -1
    assert eng.select([(dev.tree(A), ">", ("lit", 4))], idx_a=ids, n_rows_a=5, want=("a",))[0].cpu().tolist() == [1, 4]


# ============================================================ transpile(..., select_expressions=True) + execute()
KW = {"outer_joins": True, "select_expressions": True}
GOLDEN = json.load(open(os.path.join(HERE, "golden", "select_expressions.json")))


def _arrow_tables(case):
    import pyarrow as pa

    types = {"chrom": pa.string(), "start": pa.int32(), "end": pa.int32(), "name": pa.string(), "score": pa.int64(),
             "strand": pa.string(), "weight": pa.float64()}
    return {t: pa.table({c: pa.array([r[k] for r in case[t]], types[c]) for k, c in enumerate(GOLDEN["columns"])})
            for t in ("features_a", "features_b")}


def _key(r):
    return tuple((x is None, x) for x in r)


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=[c["id"] for c in GOLDEN["cases"]])
def test_execute_gives_the_golden_rows(case):
    import pyarrow as pa

    from giql_amd.execute import execute
    from giql_amd.transpile import transpile

    out = execute(transpile(case["query"], dialect="hip", **KW), _arrow_tables(case))
    assert out.column_names == ["an", "s", "bn", "e"] + case["aliases"]
    for alias in case["aliases"]:
        assert out.schema.field(alias).type in (pa.int64(), pa.float64())
    got = sorted((list(r) for r in zip(*[out.column(c).to_pylist() for c in out.column_names])), key=_key)
    want = case["rows"]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g[:4] == w[:4]
        for x, y in zip(g[4:], w[4:]):
            assert type(x) is type(y) and x == y, (case["id"], g, w)       # floats bit for bit


def _tables(seed, n_a, n_b, extra=None, span=200_000):
    """Two generated tables and their rows as numpy: (arrow tables, (chrom, start, end) per table)."""
    import pyarrow as pa

    rng = np.random.default_rng(seed)
    tables, rows = {}, {}
    for name, n in (("features_a", n_a), ("features_b", n_b)):
        start = rng.integers(0, span, n)
        end = start + rng.integers(1, 400, n)
        chrom = rng.integers(1, 4, n)
        if name == "features_a":
            chrom[: n // 50] = 9                    # a chromosome the right table lacks: unmatched rows for sure
        rows[name] = (chrom, start, end)
        cols = {"chrom": pa.array([f"chr{c}" for c in chrom]), "start": pa.array(start, pa.int32()),
                "end": pa.array(end, pa.int32()), "name": pa.array([f"{name[-1]}{i}" for i in range(n)]),
                "score": pa.array(rng.integers(0, 6, n), pa.int64(), mask=rng.random(n) < 0.2)}
        cols.update((extra or {}).get(name, {}))
        tables[name] = pa.table(cols)
    return tables, rows


def _pairs(rows):
    (ca, sa, ea), (cb, sb, eb) = rows["features_a"], rows["features_b"]
    hit = (ca[:, None] == cb[None, :]) & (sa[:, None] < eb[None, :]) & (ea[:, None] > sb[None, :])
    return np.nonzero(hit)


WO = ("SELECT a.*, b.*, (LEAST(a.end, b.end) - GREATEST(a.start, b.start)) AS overlap_bp "
      "FROM features_a a, features_b b WHERE a.interval INTERSECTS b.interval")
WAO = ("SELECT a.*, b.*, CASE WHEN b.chrom IS NULL THEN 0 "
       "ELSE LEAST(a.end, b.end) - GREATEST(a.start, b.start) END AS overlap_bp "
       "FROM features_a a LEFT JOIN features_b b ON a.interval INTERSECTS b.interval")


def test_both_recipes_as_written_against_numpy():
    """The two queries of docs/recipes/bedtools-migration.rst (-wo, -wao), stars included, on a few thousand rows."""
    import pyarrow as pa

    from giql_amd.execute import execute
    from giql_amd.transpile import transpile

    tables, rows = _tables(11, 3000, 2500)
    (ca, sa, ea), (cb, sb, eb) = rows["features_a"], rows["features_b"]
    ia, ib = _pairs(rows)
    overlap = np.minimum(ea[ia], eb[ib]) - np.maximum(sa[ia], sb[ib])
    assert len(ia) > 3000 and overlap.min() >= 1
    names = ["chrom", "start", "end", "name", "score"]
    # -wo: every pair with its overlap
    out = execute(transpile(WO, dialect="hip", select_expressions=True), tables)
    assert out.column_names == names + names + ["overlap_bp"] and out.schema.field("overlap_bp").type == pa.int64()
    assert out.column("overlap_bp").null_count == 0
    cols = [out.column(k).to_pylist() for k in (3, 8, 10)]
    assert sorted(zip(*cols)) == sorted((f"a{i}", f"b{j}", int(v)) for i, j, v in zip(ia, ib, overlap))
    # -wao: the same, plus every unmatched left row once with NULLs on the right and 0
    lone = np.setdiff1d(np.arange(len(sa)), ia)
    assert lone.size > 50
    out = execute(transpile(WAO, dialect="hip", **KW), tables)
    assert out.num_rows == len(ia) + lone.size and out.column("overlap_bp").null_count == 0
    cols = [out.column(k).to_pylist() for k in (3, 8, 10)]
    want = [(f"a{i}", f"b{j}", int(v)) for i, j, v in zip(ia, ib, overlap)] + [(f"a{i}", None, 0) for i in lone]
    assert sorted(zip(*cols), key=_key) == sorted(want, key=_key)
    assert out.column(5).null_count == lone.size                     # b.chrom is NULL exactly on the padded rows
    # without the CASE: LEAST / GREATEST skip the padded row's NULLs (DuckDB's semantics, the kernel's), so the value
    # is the left row's own length there; plain arithmetic over the right side is NULL
    q = ("SELECT a.name, b.name AS bn, LEAST(a.end, b.end) - GREATEST(a.start, b.start) AS overlap_bp, b.end - a.start AS d "
         "FROM features_a a LEFT JOIN features_b b ON a.interval INTERSECTS b.interval")
    out = execute(transpile(q, dialect="hip", **KW), tables)
    got = sorted(zip(*[out.column(c).to_pylist() for c in out.column_names]), key=_key)
    want = [(f"a{i}", f"b{j}", int(v), int(eb[j] - sa[i])) for i, j, v in zip(ia, ib, overlap)] + \
           [(f"a{i}", None, int(ea[i] - sa[i]), None) for i in lone]
    assert got == sorted(want, key=_key)


def test_left_join_with_on_and_where_residuals_order_by_limit_and_distinct():
    from giql_amd.execute import execute
    from giql_amd.transpile import transpile

    tables, rows = _tables(12, 1500, 1200)
    (ca, sa, ea), (cb, sb, eb) = rows["features_a"], rows["features_b"]
    score_a, score_b = (tables[t].column("score").to_pylist() for t in ("features_a", "features_b"))
    ia, ib = _pairs(rows)
    # ON residual: takes part in matching; WHERE residual: filters the padded result under three-valued logic
    q = ("SELECT a.name, b.name AS bn, CASE WHEN b.chrom IS NULL THEN 0 ELSE LEAST(a.end, b.end) - GREATEST(a.start, b.start) END "
         "AS overlap_bp FROM features_a a LEFT JOIN features_b b ON a.interval INTERSECTS b.interval AND b.score > a.score "
         "WHERE a.score IS NOT NULL AND (b.score IS NULL OR b.score < 5)")
    on = [(i, j) for i, j in zip(ia, ib) if score_a[i] is not None and score_b[j] is not None and score_b[j] > score_a[i]]
    matched = {i for i, _ in on}
    want = [(f"a{i}", f"b{j}", int(min(ea[i], eb[j]) - max(sa[i], sb[j]))) for i, j in on
            if score_a[i] is not None and score_b[j] < 5]
    want += [(f"a{i}", None, 0) for i in range(len(sa)) if i not in matched and score_a[i] is not None]
    out = execute(transpile(q, dialect="hip", **KW), tables)
    got = sorted(zip(*[out.column(c).to_pylist() for c in out.column_names]), key=_key)
    assert got == sorted(want, key=_key) and any(r[1] is None for r in got) and len(on) > 300
    # ORDER BY alias DESC + LIMIT
    q = ("SELECT a.name, b.name AS bn, (LEAST(a.end, b.end) - GREATEST(a.start, b.start)) AS overlap_bp "
         "FROM features_a a JOIN features_b b ON a.interval INTERSECTS b.interval ORDER BY overlap_bp DESC, a.name, bn LIMIT 25")
    overlap = np.minimum(ea[ia], eb[ib]) - np.maximum(sa[ia], sb[ib])
    every = sorted(((f"a{i}", f"b{j}", int(v)) for i, j, v in zip(ia, ib, overlap)), key=lambda r: (-r[2], r[0], r[1]))
    out = execute(transpile(q, dialect="hip", select_expressions=True), tables)
    assert list(zip(*[out.column(c).to_pylist() for c in out.column_names])) == every[:25]
    # DISTINCT over a computed column
    q = ("SELECT DISTINCT a.score, (a.end - a.start) / 100 AS hundreds FROM features_a a JOIN features_b b "
         "ON a.interval INTERSECTS b.interval")
    out = execute(transpile(q, dialect="hip", select_expressions=True), tables)
    got = sorted(zip(out.column("score").to_pylist(), out.column("hundreds").to_pylist()), key=_key)
    want = sorted({(score_a[i], float(ea[i] - sa[i]) / 100.0) for i in ia}, key=_key)
    assert got == want and len(got) < len(ia)


LEAF_KINDS = ["int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "float32", "float64", "bool"]


@pytest.mark.parametrize("kind", LEAF_KINDS)
def test_every_arrow_type_as_an_expression_leaf_with_nulls(kind):
    import pyarrow as pa

    from giql_amd.execute import execute
    from giql_amd.transpile import transpile

    rng = np.random.default_rng(700 + LEAF_KINDS.index(kind))
    n_a, n_b = 400, 350
    null = rng.random(n_a) < 0.25
    ints = {"int8": (-128, 127), "int16": (-32768, 32767), "int32": (-2**31, 2**31 - 1), "int64": (-2**61, 2**61),
            "uint8": (0, 255), "uint16": (0, 65535), "uint32": (2**31, 2**32 - 1)}
    if kind in ints:
        lo, hi = ints[kind]
        pool = [lo, hi, lo + 1, hi - 1, (lo + hi) // 2, 3]
        vals = [None if z else pool[int(rng.integers(0, len(pool)))] for z in null]
        arr = pa.array(vals, getattr(pa, kind)())
    elif kind == "bool":
        vals = [None if z else bool(rng.integers(0, 2)) for z in null]
        arr = pa.array(vals, pa.bool_())
    else:
        dt = np.float32 if kind == "float32" else np.float64
        data = np.array([0.1, -2.5, 0.0, 3.0, 1e30, 1 / 3], dt)[rng.integers(0, 6, n_a)]
        arr = pa.array(data, mask=null)
        vals = [None if z else float(x) for x, z in zip(data, null)]
    tables, rows = _tables(800 + LEAF_KINDS.index(kind), n_a, n_b, extra={"features_a": {"v": arr}}, span=30_000)
    ia, ib = _pairs(rows)
    sb = rows["features_b"][1]
    ok = np.array([v is not None for v in vals], np.uint8)
    if kind.startswith("float"):
        V = ("a", np.array([0.0 if v is None else v for v in vals], np.float64), ok)
    else:
        V = ("a", np.array([0 if v is None else int(v) for v in vals], np.int64), ok)
    S = ("b", sb.astype(np.int64))
    trees = {"x": ("+", ("*", V, ("lit", 2)), S), "y": ("if", ("isnull", V), ("lit", -1), V), "z": ("/", V, ("lit", 4))}
    q = ("SELECT a.name, b.name AS bn, a.v * 2 + b.start AS x, CASE WHEN a.v IS NULL THEN -1 ELSE a.v END AS y, a.v / 4 AS z "
         "FROM features_a a JOIN features_b b ON a.interval INTERSECTS b.interval")
    out = execute(transpile(q, dialect="hip", select_expressions=True), tables)
    assert out.num_rows == len(ia) > 300
    order = np.lexsort((ib, ia))
    got_order = sorted(range(out.num_rows), key=lambda k, an=out.column("name").to_pylist(), bn=out.column("bn").to_pylist():
                       (int(an[k][1:]), int(bn[k][1:])))
    for alias, tree in trees.items():
        vals_ref, ok_ref = R.evaluate(tree, ia[order], ib[order])
        col = out.column(alias).combine_chunks()
        assert col.type == (pa.float64() if vals_ref.dtype == np.float64 else pa.int64()), (kind, alias, col.type)
        got = col.take(pa.array(got_order)).to_pylist()
        want = [None if not o else v.item() for v, o in zip(vals_ref, ok_ref)]
        assert got == want, (kind, alias)
        assert 0 < col.null_count < out.num_rows or alias == "y"


def test_a_pinned_right_table_and_several_devices():
    from giql_amd.execute import execute, pin
    from giql_amd.transpile import transpile

    tables, rows = _tables(13, 1200, 1000)
    (ca, sa, ea), (cb, sb, eb) = rows["features_a"], rows["features_b"]
    ia, ib = _pairs(rows)
    overlap = np.minimum(ea[ia], eb[ib]) - np.maximum(sa[ia], sb[ib])
    q = ("SELECT a.name, b.name AS bn, (LEAST(a.end, b.end) - GREATEST(a.start, b.start)) AS overlap_bp "
         "FROM features_a a, features_b b WHERE a.interval INTERSECTS b.interval")
    plan = transpile(q, dialect="hip", select_expressions=True)
    want = sorted((f"a{i}", f"b{j}", int(v)) for i, j, v in zip(ia, ib, overlap))
    with pin(tables["features_b"], index=True) as pinned:
        out = execute(plan, {"features_a": tables["features_a"], "features_b": pinned})
        assert sorted(zip(*[out.column(c).to_pylist() for c in out.column_names])) == want
    # several devices: refused before a second device is touched (device 1 need not exist)
    with pytest.raises(ValueError, match="computed column is evaluated on one device"):
        execute(plan, tables, devices=[0, 1])
    with pytest.raises(ValueError, match="computed column is evaluated on one device"):
        execute(transpile(WAO, dialect="hip", **KW), tables, devices=[0, 1])
    # a query string straight into execute() takes the keyword too
    out = execute(q, tables, select_expressions=True)
    assert sorted(zip(*[out.column(c).to_pylist() for c in out.column_names])) == want


def test_execute_refuses_a_string_column_as_a_value():
    from giql_amd.execute import execute
    from giql_amd.transpile import transpile

    tables, _rows = _tables(14, 50, 40)
    q = "SELECT a.name, CASE WHEN a.score > 2 THEN b.name END AS w FROM features_a a JOIN features_b b ON a.interval INTERSECTS b.interval"
    with pytest.raises(ValueError, match="computed column"):
        execute(transpile(q, dialect="hip", select_expressions=True), tables)
