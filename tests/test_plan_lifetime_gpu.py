"""The lifetime of a plan kept in a context, cell by cell (``include/giql_hip.h``, THE LIFETIME OF A PLAN).

A context keeps at most one plan -- INNER (the within-distance plan is one), DISJOIN or CONTAINS -- between the plan
call and its fill.  The rule: the plan is consumed by its own fill and export entry points until the next call on
the context that BEGINS A CALL; six calls that use no workspace (distance, take, take_utf8_fill, mark, segment_sum and
concat_utf8_fill, STRING_AGG's byte fill, which include/giql_hip_string_agg.h adds to the five of giql_hip.h) keep an
INNER or DISJOIN plan; calls that launch nothing keep every plan.  Whether a call that begins a call then
returns at once -- an empty side, no candidates, nothing to do -- makes no difference: it has dropped the plan.

``TABLE`` below is that rule written out: one line per entry point of the ABI that takes a context (and per form of
it that returns before it claims the workspace), one word per plan.  The words come from the rule, not from a run:

* ``kept``      the fill succeeds and gives the brute-force pairs / pieces (sorted multisets);
* ``dropped``   the fill returns ``GIQL_ERR_STATE`` with its "without a successful ..." message and writes nothing
                into sentinel-filled buffers;
* ``replaced``  the column is itself a successful plan call of the row's own kind, on OTHER tables than the row's
                plan (or with an empty side): the old plan is gone like a dropped one, and the fill, which cannot
                refuse the new plan, gives the NEW plan's result -- nothing at all for the empty one.

On the INNER rows the export entry point is checked beside the fill, and ``test_export_of_a_compact_plan`` takes a
plan that HAS a compact form (a fixed-length side, no zero-length row) through every column that keeps an INNER plan:
the export succeeds there and expands to the brute-force pairs.  These tables hold rows of variable length and
zero-length rows (so that every plan has regular and irregular pairs), whose plan has no compact form: a kept plan
answers ``GIQL_ERR_STATE`` "not in the compact single-range form" (what the header promises after a within-distance
plan too), a dropped one "plan export without a successful inner_plan"; the buffers stay untouched either way.  (A new
plan without pairs exports as the header says such a plan does: ``GIQL_OK``, nothing written.)
"""

import ctypes
import functools

import numpy as np
import pytest

from oracle import pyoracle as ora

torch = pytest.importorskip("torch")

N_CHROM = 3
WINDOW = 50
ROWS = ("INNER", "WINDOW", "DISJOIN", "CONTAINS")

K, D, R = "kept", "dropped", "replaced"
ALL_KEPT, ALL_DROPPED = (K, K, K, K), (D, D, D, D)
KEEPER = (K, K, K, D)            # the six calls beside a plan: INNER and DISJOIN plans stay, a CONTAINS plan goes
INNER_PLAN = (R, R, D, D)        # a successful INNER plan call (the within-distance plan is one)

#     column                          INNER, WINDOW, DISJOIN, CONTAINS
TABLE = {
    # ---- launch nothing, or do not begin a call: every plan stays
    "get_stats":                      ALL_KEPT,
    "set_profiling":                  ALL_KEPT,
    "reserve_within_the_size":        ALL_KEPT,
    "inner_fill":                     ALL_KEPT,
    "inner_plan_export":              ALL_KEPT,
    "disjoin_fill":                   ALL_KEPT,
    "contain_fill":                   ALL_KEPT,
    "fill_from_plan":                 ALL_KEPT,
    "pairs_checksum":                 ALL_KEPT,
    "copy_probe":                     ALL_KEPT,
    "stream_probe":                   ALL_KEPT,
    "index_prepare_rows_prepared":    ALL_KEPT,     # returns before it begins a call
    "index_prepare_nearest_prepared": ALL_KEPT,
    "host_count_empty_left":          ALL_KEPT,     # giql_hip_count / giql_hip_nearest return before the device call
    "host_nearest_empty_left":        ALL_KEPT,
    "distance_no_pairs":              ALL_KEPT,     # n == 0: the keepers' ways out before they begin
    "take_no_rows":                   ALL_KEPT,
    "take_utf8_fill_no_rows":         ALL_KEPT,
    "mark_no_rows":                   ALL_KEPT,
    "concat_utf8_fill_no_rows":       ALL_KEPT,
    # ---- the six calls beside a plan
    "distance":                       KEEPER,
    "take":                           KEEPER,
    "take_utf8_fill":                 KEEPER,
    "mark":                           KEEPER,
    "segment_sum":                    KEEPER,
    "segment_sum_no_rows":            KEEPER,       # (begins its call before it looks at n)
    "concat_utf8_fill":               KEEPER,       # STRING_AGG's byte fill: begin_call_beside_plan, like take_utf8_fill
    # ---- the plan calls
    "inner_plan":                     INNER_PLAN,
    "inner_plan_empty_side":          INNER_PLAN,
    "inner_join":                     INNER_PLAN,   # plan + fill in one call: its plan stays for another fill
    "window_plan":                    INNER_PLAN,
    "window_plan_empty_side":         INNER_PLAN,
    "disjoin_plan":                   (D, D, R, D),
    "disjoin_plan_empty_target":      ALL_DROPPED,  # returns before it keeps a plan: none, not an empty one
    "contain_plan":                   (D, D, D, R),
    "contain_plan_empty_side":        (D, D, D, R),
    # ---- everything else begins a call
    "reserve_growing":                ALL_DROPPED,
    "semi":                           ALL_DROPPED,
    "semi_empty_left":                ALL_DROPPED,
    "count":                          ALL_DROPPED,
    "count_empty_left":               ALL_DROPPED,
    "nearest":                        ALL_DROPPED,
    "nearest_empty_left":             ALL_DROPPED,
    "nearest32":                      ALL_DROPPED,
    "nearest_k":                      ALL_DROPPED,
    "nearest_k_empty_left":           ALL_DROPPED,
    "semi_pred_contains":             ALL_DROPPED,
    "semi_pred_contains_empty_left":  ALL_DROPPED,
    "semi_pred_within":               ALL_DROPPED,
    "semi_pred_within_empty_left":    ALL_DROPPED,
    "semi_pred_distance":             ALL_DROPPED,
    "semi_pred_distance_empty_left":  ALL_DROPPED,
    "count_pred_contains":            ALL_DROPPED,
    "count_pred_contains_empty_left": ALL_DROPPED,
    "count_pred_within":              ALL_DROPPED,
    "count_pred_within_empty_left":   ALL_DROPPED,
    "count_pred_distance":            ALL_DROPPED,
    "count_pred_distance_empty_left": ALL_DROPPED,
    "cluster":                        ALL_DROPPED,
    "cluster_empty":                  ALL_DROPPED,
    "cluster_pred":                   ALL_DROPPED,
    "merge":                          ALL_DROPPED,
    "merge_empty":                    ALL_DROPPED,
    "merge_pred":                     ALL_DROPPED,
    "merge_agg":                      ALL_DROPPED,
    "merge_agg_empty":                ALL_DROPPED,
    "group_rows":                     ALL_DROPPED,
    "group_rows_empty":               ALL_DROPPED,
    "chrom_spans":                    ALL_DROPPED,
    "index_create":                   ALL_DROPPED,
    "index_prepare_rows":             ALL_DROPPED,
    "index_prepare_nearest":          ALL_DROPPED,
    "inner_join_indexed":             ALL_DROPPED,
    "inner_join_indexed_empty_left":  ALL_DROPPED,
    "count_indexed":                  ALL_DROPPED,
    "count_indexed_empty_left":       ALL_DROPPED,
    "semi_indexed":                   ALL_DROPPED,
    "semi_indexed_empty_left":        ALL_DROPPED,
    "nearest_indexed":                ALL_DROPPED,
    "nearest_indexed_empty_left":     ALL_DROPPED,
    "select":                         ALL_DROPPED,
    "select_no_candidates":           ALL_DROPPED,
    "select_expr":                    ALL_DROPPED,
    "eval_expr":                      ALL_DROPPED,
    "eval_expr_no_candidates":        ALL_DROPPED,
    "take_utf8_plan":                 ALL_DROPPED,
    "take_utf8_plan_no_rows":         ALL_DROPPED,
    "left_pad":                       ALL_DROPPED,
    "left_pad_no_pairs":              ALL_DROPPED,
    "host_inner":                     ALL_DROPPED,  # (its own plans read columns it staged and released: none stays)
    "host_semi_anti":                 ALL_DROPPED,
    "host_count":                     ALL_DROPPED,
    "host_nearest":                   ALL_DROPPED,
    # ---- the extension headers' entry points: each begins a call before its first way out
    "range_set_any":                  ALL_DROPPED,
    "range_set_any_no_rows":          ALL_DROPPED,
    "merge_str":                      ALL_DROPPED,  # giql_hip_merge_dev_impl's begin_call, as merge / merge_agg
    "merge_str_empty":                ALL_DROPPED,
    "pair_agg":                       ALL_DROPPED,  # pair_agg_impl begins its call before its own checks
    "pair_agg_no_pairs":              ALL_DROPPED,
    "pair_expr_agg":                  ALL_DROPPED,
    "coverage":                       ALL_DROPPED,  # begin_call, then the way out with no rows, then claim_arena
    "coverage_empty":                 ALL_DROPPED,
}
CELLS = [(row, col) for col in TABLE for row in ROWS]
SENTINEL = -7
MESSAGES = {"INNER": b"inner_fill without a successful inner_plan", "WINDOW": b"inner_fill without a successful inner_plan",
            "DISJOIN": b"disjoin_fill without a successful disjoin_plan",
            "CONTAINS": b"contain_fill without a successful contain_plan"}
EXPORT_DROPPED = b"plan export without a successful inner_plan"
EXPORT_KEPT = b"not in the compact single-range form"


NO_CONTEXT = {"abi_version", "last_error", "device_count", "free_host", "host_pool_trim", "index_destroy", "index_info"}
COLUMN_OF = {   # entry point (without giql_hip_ and _dev) -> its first column; create / destroy make and end the context
    "create": None, "destroy": None, "reserve": "reserve_growing", "set_profiling": "set_profiling", "get_stats": "get_stats",
    "inner_plan": "inner_plan", "inner_fill": "inner_fill", "semi_anti": "semi", "count": "count", "nearest": "nearest",
    "chrom_spans": "chrom_spans", "host:inner": "host_inner", "host:semi_anti": "host_semi_anti", "host:count": "host_count",
    "host:nearest": "host_nearest", "pairs_checksum": "pairs_checksum", "take": "take", "take_utf8_plan": "take_utf8_plan",
    "take_utf8_fill": "take_utf8_fill", "select": "select", "select_expr": "select_expr", "mark": "mark",
    "cluster": "cluster", "cluster_pred": "cluster_pred", "merge": "merge", "merge_pred": "merge_pred",
    "group_rows": "group_rows", "segment_sum": "segment_sum", "inner_join": "inner_join",
    "inner_plan_export": "inner_plan_export", "fill_from_plan": "fill_from_plan", "copy_probe": "copy_probe",
    "nearest_k": "nearest_k", "stream_probe": "stream_probe", "nearest32": "nearest32", "index_create": "index_create",
    "inner_join_indexed": "inner_join_indexed", "disjoin_plan": "disjoin_plan", "disjoin_fill": "disjoin_fill",
    "contain_plan": "contain_plan", "contain_fill": "contain_fill", "window_plan": "window_plan", "distance": "distance",
    "index_prepare_rows": "index_prepare_rows", "count_indexed": "count_indexed", "semi_anti_indexed": "semi_indexed",
    "index_prepare_nearest": "index_prepare_nearest", "nearest_indexed": "nearest_indexed", "left_pad": "left_pad",
    "semi_anti_pred": "semi_pred_contains", "count_pred": "count_pred_contains", "eval_expr": "eval_expr",
    "merge_agg": "merge_agg", "range_set_any": "range_set_any", "merge_str": "merge_str",
    "concat_utf8_fill": "concat_utf8_fill", "pair_agg": "pair_agg", "pair_expr_agg": "pair_expr_agg", "coverage": "coverage",
}


def test_the_table_is_complete():
    """CPU: a column for every entry point of the ABI that takes a context, the early-return forms the rule is
    about, and nothing in a cell but the three words, where the rule allows each."""
    from _stream_harness import abi_symbols

    missing = []
    for s in abi_symbols():       # every ``..._SYMBOLS`` list of ``_lib``: the extension headers' entry points too
        name = s[len("giql_hip_"):]
        if name in NO_CONTEXT:
            continue
        key = name[:-4] if name.endswith("_dev") else "host:" + name if name in ("inner", "semi_anti", "count", "nearest") else name
        if key not in COLUMN_OF:
            missing.append(key)
            continue
        assert COLUMN_OF[key] is None or COLUMN_OF[key] in TABLE, s
    assert not missing, f"entry points that take a context and have no column in TABLE: {missing}"
    assert {w for words in TABLE.values() for w in words} == {K, D, R}
    for needed in ("semi", "count", "nearest", "nearest_k", "semi_pred_contains", "semi_pred_within", "semi_pred_distance",
                   "count_pred_contains", "count_pred_within", "count_pred_distance", "count_indexed", "semi_indexed",
                   "nearest_indexed"):
        assert needed in TABLE and needed + "_empty_left" in TABLE, needed
    for needed in ("cluster_empty", "merge_empty", "merge_agg_empty", "group_rows_empty", "inner_plan_empty_side",
                   "window_plan_empty_side", "contain_plan_empty_side", "disjoin_plan_empty_target", "select_no_candidates",
                   "eval_expr_no_candidates", "take_utf8_plan_no_rows", "left_pad_no_pairs", "index_prepare_rows_prepared",
                   "range_set_any_no_rows", "merge_str_empty", "concat_utf8_fill_no_rows", "pair_agg_no_pairs", "coverage_empty"):
        assert needed in TABLE, needed
    # the rule, restated: only a plan call replaces, and only on rows of its own kind; only the six calls beside a
    # plan tell a CONTAINS plan from the others; everything else is one word for all four plans
    for col, words in TABLE.items():
        if R in words:
            assert col in REPLACED_BY and words in (INNER_PLAN, (D, D, R, D), (D, D, D, R)), col
        elif words == KEEPER:
            assert col in ("distance", "take", "take_utf8_fill", "mark", "segment_sum", "segment_sum_no_rows",
                           "concat_utf8_fill"), col
        else:
            assert words in (ALL_KEPT, ALL_DROPPED), col


# ---------------------------------------------------------------- tables and their brute-force answers
def _table(seed, n, regular=False):
    """n rows on three chromosomes inside 6,000 positions, 1 to 300 long; a few zero-length unless ``regular``."""
    r = np.random.default_rng(seed)
    ch = r.integers(0, N_CHROM, n).astype(np.int32)
    st = r.integers(0, 6000, n).astype(np.int32)
    ln = r.integers(1, 300, n).astype(np.int32)
    if not regular:
        ln[r.choice(n, 6, replace=False)] = 0
    return ora.Side(ch, st, st + ln)


@functools.lru_cache(maxsize=None)
def tables():
    u = _table(904, 300, regular=True)
    u.end[:] = u.start + 100                        # one length, no zero-length row: INNER plans over it are compact
    return {"a": _table(901, 200), "b": _table(902, 300), "q": _table(903, 150, regular=True), "u": u}


def _i64(s):
    return s.chrom.astype(np.int64), s.cs.astype(np.int64), s.ce.astype(np.int64)


@functools.lru_cache(maxsize=None)
def truth(kind, first, second):
    """The sorted result of a plan of ``kind`` over tables()[first], tables()[second]."""
    import _contain_ref
    import _disjoin_ref
    import _distance_ref

    x, y = tables()[first], tables()[second]
    if kind == "INNER":
        return ora.sort_pairs(*ora.c_inner(x, y, "sweep"))
    if kind == "WINDOW":
        return _distance_ref.window_pairs(*_i64(x), *_i64(y), WINDOW)
    if kind == "DISJOIN":
        return _disjoin_ref.brute_force_arrays(*_i64(x), *_i64(y))
    return _contain_ref.contain_pairs(*_i64(x), *_i64(y))


def test_every_plan_has_regular_and_irregular_pairs():
    """CPU: each of the four results is non-empty, and holds rows of zero-length parents as well as regular ones."""
    t = tables()
    zero = {k: s.ce == s.cs for k, s in t.items()}
    assert zero["a"].sum() == 6 and zero["b"].sum() == 6 and not zero["q"].any()
    for kind in ("INNER", "WINDOW", "CONTAINS"):
        p = truth(kind, "a", "b")
        irregular = zero["a"][p[:, 0]] | zero["b"][p[:, 1]]
        assert irregular.any() and (~irregular).sum() > 100, kind
    assert truth("DISJOIN", "a", "b").shape[0] > 100
    for kind in ROWS:           # the plan columns run on the tables exchanged: another result, so a stale fill shows
        assert not np.array_equal(truth(kind, "a", "b"), truth(kind, "b", "a")), kind
        assert truth(kind, "a", "b").shape[0] < 4096 and truth(kind, "b", "a").shape[0] < 4096
    assert not np.array_equal(truth("INNER", "a", "b"), truth("WINDOW", "a", "b"))


# ---------------------------------------------------------------- one context and everything the columns need
class Fixture:
    def __init__(self):
        from giql_amd import _lib
        from giql_amd.engine import HipEngine
        from test_context_transitions import _dev

        self.lib = _lib
        self.eng = HipEngine(0)
        self.L, self.h = self.eng._L, self.eng._h
        self.dev = {k: _dev(s) for k, s in tables().items()}
        self.side = {k: d.c_struct() for k, d in self.dev.items()}
        self.side["none"] = _lib.CSide(None, None, None, 0, 0, 0)
        self.n = {k: s.n for k, s in tables().items()}
        cu = dict(device="cuda:0")
        big = 4096
        self.i32 = [torch.zeros(big, dtype=torch.int32, **cu) for _ in range(4)]
        self.i64 = [torch.zeros(big, dtype=torch.int64, **cu) for _ in range(2)]
        self.u8 = torch.zeros(big, dtype=torch.uint8, **cu)
        self.iota = torch.arange(big, dtype=torch.int32, **cu)
        self.zeros4 = torch.zeros(4, dtype=torch.int32, **cu)
        self.mib = [torch.zeros(1 << 18, dtype=torch.int32, **cu) for _ in range(2)]     # the stream probe's least size
        # a string column of 40 rows and the offsets of a take of 64 of them (made by a plan call, once, up front)
        words = [f"w{i}" * (i % 5) for i in range(40)]
        self.utf8_off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(w) for w in words])]).astype(np.int32)).to("cuda:0")
        self.utf8_data = torch.from_numpy(np.frombuffer("".join(words).encode(), np.uint8).copy()).to("cuda:0")
        self.utf8_idx = torch.from_numpy(np.random.default_rng(5).integers(0, 40, 64).astype(np.int32)).to("cuda:0")
        self.utf8_out_off = torch.zeros(65, dtype=torch.int32, **cu)
        self.utf8_out = torch.zeros(4096, dtype=torch.uint8, **cu)
        assert self.take_utf8_plan(64) == 0
        # an index over the regular table, prepared for the row operators and for NEAREST
        self.index = self.index_create()
        assert self.L.giql_hip_index_prepare_rows_dev(self.h, self.index, self.st()) == 0
        assert self.L.giql_hip_index_prepare_nearest_dev(self.h, self.index, self.st()) == 0
        self.pred = (_lib.CPred * 1)(_lib.CPred(
            _lib.COperand(_lib.SIDE_A, _lib.T_I32, self.dev["a"].start.data_ptr(), None, 0, 0.0, 0, 0),
            _lib.COperand(_lib.SIDE_LIT, 0, None, None, 0, 0.0, 0, 0), _lib.OPS[">="], 0))
        self.node = (_lib.COperand * 1)(_lib.COperand(_lib.SIDE_A, _lib.T_I32, self.dev["a"].start.data_ptr(), None, 0, 0.0, 0, 0))
        self.expr_out = (_lib.CExprOut * 1)(_lib.CExprOut(0, 1, _lib.T_I64, 0, self.i64[0].data_ptr(), None))
        self.agg = (_lib.CAgg * 1)(_lib.CAgg(_lib.AGG_FUNCS["COUNT"], _lib.T_I32, self.dev["a"].start.data_ptr(), None,
                                             self.i64[1].data_ptr(), None))

    def close(self):
        self.L.giql_hip_index_destroy(self.index)
        self.eng.close()

    def st(self):
        return self.eng._stream()

    def ref(self, name):
        return ctypes.byref(self.side[name])

    def p(self, t):
        return t.data_ptr()

    # ---- the plans and their fills (rows)
    def plan(self, kind, first="a", second="b"):
        """(return code, count) of a plan of ``kind`` over the named tables."""
        n = ctypes.c_int64(-1)
        x, y, L, h = self.ref(first), self.ref(second), self.L, self.h
        if kind == "INNER":
            rc = L.giql_hip_inner_plan_dev(h, x, y, N_CHROM, self.st(), ctypes.byref(n))
        elif kind == "WINDOW":
            rc = L.giql_hip_window_plan_dev(h, x, y, N_CHROM, WINDOW, self.st(), ctypes.byref(n))
        elif kind == "DISJOIN":
            rc = L.giql_hip_disjoin_plan_dev(h, x, y, N_CHROM, ctypes.byref(n), self.st())
        else:
            rc = L.giql_hip_contain_plan_dev(h, x, y, N_CHROM, self.st(), ctypes.byref(n))
        return rc, int(n.value)

    def fill(self, kind, cap):
        """(return code, the sentinel-filled output tensors) of the fill of ``kind`` with room for ``cap``."""
        outs = [torch.full((cap + 8,), SENTINEL, dtype=torch.int32, device="cuda:0") for _ in range(3 if kind == "DISJOIN" else 2)]
        ptr = [o.data_ptr() for o in outs]
        if kind in ("INNER", "WINDOW"):
            rc = self.L.giql_hip_inner_fill_dev(self.h, ptr[0], ptr[1], cap, self.st())
        elif kind == "DISJOIN":
            rc = self.L.giql_hip_disjoin_fill_dev(self.h, ptr[0], ptr[1], ptr[2], cap, self.st())
        else:
            rc = self.L.giql_hip_contain_fill_dev(self.h, ptr[0], ptr[1], cap, self.st())
        return rc, outs

    def export(self):
        """(return code, message, output tensors) of giql_hip_inner_plan_export_dev into sentinel-filled buffers."""
        outs = [torch.full((512,), SENTINEL, dtype=torch.int32, device="cuda:0") for _ in range(4)]
        qia, nq, ns = ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int64(0)
        rc = self.L.giql_hip_inner_plan_export_dev(self.h, *(o.data_ptr() for o in outs), 512, 512, 0, 0, ctypes.byref(qia),
                                                   ctypes.byref(nq), ctypes.byref(ns), self.st())
        return rc, self.L.giql_hip_last_error(), outs

    # ---- helpers of the columns
    def take_utf8_plan(self, n):
        nb = ctypes.c_int64(-1)
        return self.L.giql_hip_take_utf8_plan_dev(self.h, self.p(self.utf8_off), 40, self.p(self.utf8_idx), n,
                                                  self.p(self.utf8_out_off), ctypes.byref(nb), self.st())

    def index_create(self):
        handle = ctypes.c_void_p()
        assert self.L.giql_hip_index_create_dev(self.h, self.ref("q"), N_CHROM, self.st(), ctypes.byref(handle)) == 0
        return handle

    def workspace_bytes(self):
        st = self.lib.CStats()
        assert self.L.giql_hip_get_stats(self.h, ctypes.byref(st)) == 0
        return int(st.workspace_bytes)


@pytest.fixture(scope="module")
def fx():
    f = Fixture()
    yield f
    f.close()


def _columns(f):
    """column -> a callable that makes the call and returns its status (asserted 0 by the test unless the column is
    one of FILLS_OF_OTHER_PLANS, whose status depends on the row)."""
    L, h, st, p, ref = f.L, f.h, f.st, f.p, f.ref
    na, nq = f.n["a"], f.n["q"]
    i32, i64, u8 = f.i32, f.i64, f.u8
    n64 = ctypes.c_int64
    out = {}

    def col(fn):
        out[fn.__name__] = fn
        return fn

    def both(name, call):
        """``name`` on the tables and ``name``_empty_left with no left row."""
        out[name] = lambda: call("a", na)
        out[name + "_empty_left"] = lambda: call("none", 0)

    # -- launch nothing / begin no call
    out["get_stats"] = lambda: L.giql_hip_get_stats(h, ctypes.byref(f.lib.CStats()))
    out["set_profiling"] = lambda: L.giql_hip_set_profiling(h, 0)
    out["reserve_within_the_size"] = lambda: L.giql_hip_reserve(h, max(f.workspace_bytes(), 1))
    out["reserve_growing"] = lambda: L.giql_hip_reserve(h, f.workspace_bytes() + (1 << 20))
    out["inner_fill"] = lambda: f.fill("INNER", 1 << 16)[0]
    out["disjoin_fill"] = lambda: f.fill("DISJOIN", 1 << 16)[0]
    out["contain_fill"] = lambda: f.fill("CONTAINS", 1 << 16)[0]
    out["inner_plan_export"] = lambda: f.export()[0]

    @col
    def fill_from_plan():     # a hand-made compact plan: query row 0 matches sorted rows 0 and 1
        q_rid, lo, cnt, s_rid = (torch.tensor(v, dtype=torch.int32, device="cuda:0") for v in ([0], [0], [2], [5, 6]))
        n = n64(-1)
        rc = L.giql_hip_fill_from_plan_dev(h, p(q_rid), p(lo), p(cnt), 1, p(s_rid), 2, p(i32[0]), p(i32[1]), 64, -1, st(),
                                           ctypes.byref(n))
        assert n.value == 2 and i32[1][:2].tolist() == [5, 6]
        return rc

    @col
    def pairs_checksum():
        s = ctypes.c_uint64(0)
        return L.giql_hip_pairs_checksum_dev(h, p(f.iota), p(f.iota), 64, st(), ctypes.byref(s))

    @col
    def copy_probe():
        g = ctypes.c_double(0)
        return L.giql_hip_copy_probe_dev(h, p(f.iota), p(i32[0]), 4096 * 4, 1, st(), ctypes.byref(g))

    @col
    def stream_probe():
        g = ctypes.c_double(0)
        return L.giql_hip_stream_probe_dev(h, p(f.mib[0]), p(f.mib[1]), 1 << 20, 2, 1, 0, 1, 1, st(), ctypes.byref(g))

    out["index_prepare_rows_prepared"] = lambda: L.giql_hip_index_prepare_rows_dev(h, f.index, st())
    out["index_prepare_nearest_prepared"] = lambda: L.giql_hip_index_prepare_nearest_dev(h, f.index, st())

    # -- the calls beside a plan, and their ways out with nothing to do
    def distance(n):
        return L.giql_hip_distance_dev(h, ref("a"), ref("b"), p(f.zeros4), p(f.zeros4), n, None, None, 0, p(i64[0]), p(u8), st())

    def take(n):
        cols = (ctypes.c_void_p * 1)(f.dev["a"].start.data_ptr())
        outs = (ctypes.c_void_p * 1)(p(i32[0]))
        return L.giql_hip_take_dev(h, cols, (ctypes.c_int32 * 1)(4), 1, na, p(f.iota), n, outs, st())

    def take_utf8_fill(n):
        return L.giql_hip_take_utf8_fill_dev(h, p(f.utf8_off), p(f.utf8_data), 40, p(f.utf8_idx), n, p(f.utf8_out_off),
                                             p(f.utf8_out), st())

    def segment_sum(n):
        return L.giql_hip_segment_sum_dev(h, p(i64[0]), p(f.zeros4), n, p(i64[1]), 1, st())

    out.update({"distance": lambda: distance(4), "distance_no_pairs": lambda: distance(0),
                "take": lambda: take(na), "take_no_rows": lambda: take(0),
                "take_utf8_fill": lambda: take_utf8_fill(64), "take_utf8_fill_no_rows": lambda: take_utf8_fill(0),
                "mark": lambda: L.giql_hip_mark_dev(h, p(f.zeros4), 4, p(u8), na, st()),
                "mark_no_rows": lambda: L.giql_hip_mark_dev(h, p(f.zeros4), 0, p(u8), na, st()),
                "segment_sum": lambda: segment_sum(4), "segment_sum_no_rows": lambda: segment_sum(0)})

    # -- the plan calls: on the tables exchanged, so that a fill that still answers for the row's plan shows
    def planned(kind, first, second):
        def call():
            rc, n = f.plan(kind, first, second)
            assert n == truth(kind, first, second).shape[0] if "none" not in (first, second) else n == 0, (kind, n)
            return rc
        return call

    out.update({"inner_plan": planned("INNER", "b", "a"), "inner_plan_empty_side": planned("INNER", "a", "none"),
                "window_plan": planned("WINDOW", "b", "a"), "window_plan_empty_side": planned("WINDOW", "none", "b"),
                "disjoin_plan": planned("DISJOIN", "b", "a"), "disjoin_plan_empty_target": planned("DISJOIN", "none", "b"),
                "contain_plan": planned("CONTAINS", "b", "a"), "contain_plan_empty_side": planned("CONTAINS", "a", "none")})

    @col
    def inner_join():
        n = n64(-1)
        rc = L.giql_hip_inner_join_dev(h, ref("b"), ref("a"), N_CHROM, p(i32[0]), p(i32[1]), 4096, st(), ctypes.byref(n))
        assert n.value == truth("INNER", "b", "a").shape[0]
        return rc

    # -- the operators
    both("semi", lambda a, n: L.giql_hip_semi_anti_dev(h, ref(a), ref("b"), N_CHROM, 0, p(i32[0]), ctypes.byref(n64()), st()))
    both("count", lambda a, n: L.giql_hip_count_dev(h, ref(a), ref("b"), N_CHROM, p(i64[0]), st()))
    both("nearest", lambda a, n: L.giql_hip_nearest_dev(h, ref(a), ref("b"), N_CHROM, 0, -1, p(i32[0]), p(i64[0]), st()))
    out["nearest32"] = lambda: L.giql_hip_nearest32_dev(h, ref("a"), ref("b"), N_CHROM, 0, -1, p(i32[0]), st())
    both("nearest_k", lambda a, n: L.giql_hip_nearest_k_dev(h, ref(a), ref("b"), N_CHROM, 2, 0, -1, p(i32[0]), p(i64[0]), st()))
    for word, code in (("contains", f.lib.ROWPRED_CONTAINS), ("within", f.lib.ROWPRED_WITHIN), ("distance", f.lib.ROWPRED_DISTANCE)):
        both("semi_pred_" + word, lambda a, n, code=code: L.giql_hip_semi_anti_pred_dev(
            h, ref(a), ref("b"), N_CHROM, code, WINDOW, 0, p(i32[0]), ctypes.byref(n64()), st()))
        both("count_pred_" + word, lambda a, n, code=code: L.giql_hip_count_pred_dev(
            h, ref(a), ref("b"), N_CHROM, code, WINDOW, p(i64[0]), st()))

    def one_table(name, call):
        out[name] = lambda: call("a")
        out[name + "_empty"] = lambda: call("none")

    one_table("cluster", lambda s: L.giql_hip_cluster_dev(h, ref(s), N_CHROM, 0, p(i64[0]), st()))
    out["cluster_pred"] = lambda: L.giql_hip_cluster_pred_dev(h, ref("a"), N_CHROM, 0, f.pred, 1, p(i64[0]), st())
    merge_outs = lambda: (p(i32[0]), p(i32[1]), p(i32[2]), p(i64[0]), 4096, ctypes.byref(n64()), st())
    one_table("merge", lambda s: L.giql_hip_merge_dev(h, ref(s), N_CHROM, 0, *merge_outs()))
    out["merge_pred"] = lambda: L.giql_hip_merge_pred_dev(h, ref("a"), N_CHROM, 0, f.pred, 1, *merge_outs())
    one_table("merge_agg", lambda s: L.giql_hip_merge_agg_dev(h, ref(s), N_CHROM, 0, None, 0, f.agg, 1, *merge_outs()))
    one_table("group_rows", lambda s: L.giql_hip_group_rows_dev(h, ref(s), N_CHROM, p(i32[0]), p(i32[1]), ctypes.byref(n64()), st()))

    @col
    def chrom_spans():
        spans = np.zeros(N_CHROM, np.int64)
        return L.giql_hip_chrom_spans_dev(h, ref("a"), ref("b"), N_CHROM, spans.ctypes.data, st())

    # -- the index entry points
    @col
    def index_create():
        return L.giql_hip_index_destroy(f.index_create())

    def fresh_index(prepare):
        def call():
            handle = f.index_create()
            rc = prepare(h, handle, st())
            L.giql_hip_index_destroy(handle)
            return rc
        return call

    out["index_prepare_rows"] = fresh_index(L.giql_hip_index_prepare_rows_dev)
    out["index_prepare_nearest"] = fresh_index(L.giql_hip_index_prepare_nearest_dev)
    indexed = lambda name, call: out.update({name: lambda: call("q"), name + "_empty_left": lambda: call("none")})
    indexed("inner_join_indexed", lambda a: L.giql_hip_inner_join_indexed_dev(h, f.index, ref(a), p(i32[0]), p(i32[1]), 4096, st(),
                                                                              ctypes.byref(n64())))
    indexed("count_indexed", lambda a: L.giql_hip_count_indexed_dev(h, f.index, ref(a), p(i64[0]), st()))
    indexed("semi_indexed", lambda a: L.giql_hip_semi_anti_indexed_dev(h, f.index, ref(a), 0, p(i32[0]), ctypes.byref(n64()), st()))
    indexed("nearest_indexed", lambda a: L.giql_hip_nearest_indexed_dev(h, f.index, ref(a), 0, -1, p(i32[0]), p(i64[0]), st()))

    # -- residual filters, computed columns, projections, the pad
    def select(n):
        return L.giql_hip_select_dev(h, f.pred, 1, None, na, None, 0, n, p(i32[0]), None, ctypes.byref(n64()), st())

    def eval_expr(n):
        return L.giql_hip_eval_expr_dev(h, f.node, 1, f.expr_out, 1, None, na, None, 0, n, None, st())

    def left_pad(n_pairs, n_rows):
        i32[0][:4] = 0
        return L.giql_hip_left_pad_dev(h, p(i32[0]), p(i32[1]), n_pairs, 4096, n_rows, st(), ctypes.byref(n64()))

    out.update({"select": lambda: select(na), "select_no_candidates": lambda: select(0),
                "select_expr": lambda: L.giql_hip_select_expr_dev(h, f.pred, 1, None, 0, None, na, None, 0, na, p(i32[0]), None,
                                                                  ctypes.byref(n64()), st()),
                "eval_expr": lambda: eval_expr(na), "eval_expr_no_candidates": lambda: eval_expr(0),
                "take_utf8_plan": lambda: f.take_utf8_plan(64), "take_utf8_plan_no_rows": lambda: f.take_utf8_plan(0),
                "left_pad": lambda: left_pad(4, na), "left_pad_no_pairs": lambda: left_pad(0, 0)})

    # -- the extension headers: literal range sets, STRING_AGG beside MERGE, the pair aggregates, coverage
    cu = dict(device="cuda:0")
    set_out = [torch.zeros(4096, dtype=torch.uint8, **cu) for _ in range(2)]
    set_host = (np.array([0], np.int32), np.array([3000], np.int64), np.array([1000], np.int64))     # chrom 0, [1000, 3000)
    sets = (f.lib.CRangeSet * 1)(f.lib.CRangeSet(f.lib.RANGE_OPS["intersects"], 1, set_host[0].ctypes.data,
                                                 set_host[1].ctypes.data, set_host[2].ctypes.data, p(set_out[0]), p(set_out[1])))

    def range_set_any(n, _alive=(set_host, set_out)):      # (the struct points into both: they live as long as it does)
        d = f.dev["a"]
        return L.giql_hip_range_set_any_dev(h, p(d.chrom), p(d.start), p(d.end), None, None, None, n, sets, 1, st())

    # a string column over table "a"; one merge_str up front leaves the order and the destinations the fill reads
    names = [b"n%d" % i * (i % 4) for i in range(na)]
    name_off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(w) for w in names])]).astype(np.int32)).to("cuda:0")
    name_data = torch.from_numpy(np.frombuffer(b"".join(names), np.uint8).copy()).to("cuda:0")
    str_out = torch.zeros(1 << 16, dtype=torch.uint8, **cu)

    def str_bufs():
        return {"off": torch.zeros(4097, dtype=torch.int32, **cu), "nn": torch.zeros(4096, dtype=torch.int64, **cu),
                "dst": torch.zeros(4096, dtype=torch.int32, **cu), "order": torch.zeros(4096, dtype=torch.int32, **cu)}

    def merge_str(s, b):
        strs = (f.lib.CStrAgg * 1)(f.lib.CStrAgg(p(name_off), None, 1, p(b["off"]), p(b["nn"]), p(b["dst"]), -7))
        rc = L.giql_hip_merge_str_dev(h, ref(s), N_CHROM, 0, None, 0, None, 0, strs, 1, p(i32[0]), p(i32[1]), p(i32[2]), p(i64[0]),
                                      p(b["order"]), 4096, ctypes.byref(n64()), st())
        return rc, int(strs[0].n_bytes)

    kept_str, scratch_str = str_bufs(), str_bufs()
    rc, n_bytes = merge_str("a", kept_str)
    assert rc == 0 and 0 < n_bytes <= str_out.numel(), (rc, n_bytes, L.giql_hip_last_error())

    def concat_utf8_fill(n):
        return L.giql_hip_concat_utf8_fill_dev(h, p(name_off), p(name_data), na, p(kept_str["order"]), p(kept_str["dst"]), n,
                                               b",", 1, p(str_out), st())

    expr_agg = (f.lib.CPairExprAgg * 1)(f.lib.CPairExprAgg(f.lib.AGG_FUNCS["SUM"], f.lib.T_I64, None, None, 0, 1,
                                                           p(i64[1]), None))

    def pair_agg(n_pairs):      # COUNT over a column of B: four pairs (row 0, row 0), or none
        return L.giql_hip_pair_agg_dev(h, p(f.zeros4), p(f.zeros4), n_pairs, na, f.n["b"], f.agg, 1, p(i64[0]), st())

    def coverage(s):
        return L.giql_hip_coverage_dev(h, ref(s), N_CHROM, 0, p(i32[0]), p(i32[1]), p(i32[2]), p(i64[0]), 4096,
                                       ctypes.byref(n64()), st())

    out.update({"range_set_any": lambda: range_set_any(na), "range_set_any_no_rows": lambda: range_set_any(0),
                "merge_str": lambda: merge_str("a", scratch_str)[0], "merge_str_empty": lambda: merge_str("none", scratch_str)[0],
                "concat_utf8_fill": lambda: concat_utf8_fill(na), "concat_utf8_fill_no_rows": lambda: concat_utf8_fill(0),
                "pair_agg": lambda: pair_agg(4), "pair_agg_no_pairs": lambda: pair_agg(0),
                "pair_expr_agg": lambda: L.giql_hip_pair_expr_agg_dev(h, p(f.zeros4), p(f.zeros4), 4, na, f.n["b"], f.node, 1,
                                                                      expr_agg, 1, p(i64[0]), st()),
                "coverage": lambda: coverage("a"), "coverage_empty": lambda: coverage("none")})

    # -- the host-buffer entry points (host columns in, library-owned or caller-owned host results out)
    t = tables()
    host = {k: f.lib.CSide(s.chrom.ctypes.data, s.start.ctypes.data, s.end.ctypes.data, s.n, 0, 0) for k, s in t.items()}
    host["none"] = f.side["none"]
    hb = lambda k: ctypes.byref(host[k])
    h_i32, h_i64 = np.zeros(na, np.int32), np.zeros(na, np.int64)

    @col
    def host_inner():
        n, ra, rb = n64(-1), ctypes.c_void_p(), ctypes.c_void_p()
        rc = L.giql_hip_inner(h, hb("a"), hb("b"), N_CHROM, ctypes.byref(n), ctypes.byref(ra), ctypes.byref(rb))
        assert n.value == truth("INNER", "a", "b").shape[0]
        L.giql_hip_free_host(ra)
        L.giql_hip_free_host(rb)
        return rc

    @col
    def host_semi_anti():
        n, rows = n64(-1), ctypes.c_void_p()
        rc = L.giql_hip_semi_anti(h, hb("a"), hb("b"), N_CHROM, 0, ctypes.byref(n), ctypes.byref(rows))
        L.giql_hip_free_host(rows)
        return rc

    out.update({"host_count": lambda: L.giql_hip_count(h, hb("a"), hb("b"), N_CHROM, h_i64.ctypes.data),
                "host_count_empty_left": lambda: L.giql_hip_count(h, hb("none"), hb("b"), N_CHROM, h_i64.ctypes.data),
                "host_nearest": lambda: L.giql_hip_nearest(h, hb("a"), hb("b"), N_CHROM, 0, -1, h_i32.ctypes.data, h_i64.ctypes.data),
                "host_nearest_empty_left": lambda: L.giql_hip_nearest(h, hb("none"), hb("b"), N_CHROM, 0, -1, h_i32.ctypes.data,
                                                                      h_i64.ctypes.data)})
    return out


FILLS_OF_OTHER_PLANS = {"inner_fill": ("INNER", "WINDOW"), "inner_plan_export": (), "disjoin_fill": ("DISJOIN",),
                        "contain_fill": ("CONTAINS",)}       # column -> the rows on which it returns 0
REPLACED_BY = {"inner_plan": ("INNER", "b", "a"), "inner_join": ("INNER", "b", "a"), "window_plan": ("WINDOW", "b", "a"),
               "disjoin_plan": ("DISJOIN", "b", "a"), "contain_plan": ("CONTAINS", "b", "a"),
               "inner_plan_empty_side": None, "window_plan_empty_side": None, "contain_plan_empty_side": None}


@pytest.fixture(scope="module")
def columns(fx):
    cols = _columns(fx)
    assert sorted(cols) == sorted(TABLE), sorted(set(cols) ^ set(TABLE))
    return cols


def _result(kind, outs, n):
    got = np.stack([o[:n].cpu().numpy() for o in outs], 1).astype(np.int64)
    return got[np.lexsort(tuple(got[:, k] for k in range(got.shape[1] - 1, -1, -1)))]


def _untouched(outs):
    return all(int((o != SENTINEL).sum()) == 0 for o in outs)


@pytest.mark.gpu
@pytest.mark.parametrize("row,col", CELLS, ids=[f"{r}-{c}" for r, c in CELLS])
def test_cell(fx, columns, row, col):
    word = TABLE[col][ROWS.index(row)]
    want = truth(row, "a", "b")
    rc, n = fx.plan(row)
    assert (rc, n) == (0, want.shape[0]), (row, "plan", rc, n, fx.L.giql_hip_last_error())
    status = columns[col]()
    if col in FILLS_OF_OTHER_PLANS:
        expect = 0 if row in FILLS_OF_OTHER_PLANS[col] else fx.lib.GIQL_ERR_STATE
        assert status == expect, (row, col, status, fx.L.giql_hip_last_error())
    else:
        assert status == 0, (row, col, status, fx.L.giql_hip_last_error())
    new = REPLACED_BY[col] if word == R else None
    inner = row in ("INNER", "WINDOW")
    if inner:
        x_rc, x_msg, x_outs = fx.export()
        assert _untouched(x_outs), (row, col, "export wrote")
        if word == R and new is None:       # an INNER plan without pairs exports as such: GIQL_OK, nothing written
            assert x_rc == 0, (row, col, "export", x_rc, x_msg)
        else:
            assert x_rc == fx.lib.GIQL_ERR_STATE, (row, col, "export", x_rc, x_msg)
            assert (EXPORT_DROPPED if word == D else EXPORT_KEPT) in x_msg, (row, col, "export", x_msg)
    if new is not None:         # the fill of the new plan needs the new plan's room
        n = truth(*new).shape[0]
    rc, outs = fx.fill(row, n)
    if word == K:
        assert rc == 0, (row, col, "the plan was dropped", fx.L.giql_hip_last_error())
        assert np.array_equal(_result(row, outs, n), want), (row, col, "the kept plan's fill")
        assert _untouched([o[n:] for o in outs])
    elif word == D:
        assert rc == fx.lib.GIQL_ERR_STATE, (row, col, "the plan was kept", rc)
        assert MESSAGES[row] in fx.L.giql_hip_last_error(), (row, col, fx.L.giql_hip_last_error())
        assert _untouched(outs), (row, col, "a refused fill wrote")
    else:
        assert word == R and rc == 0, (row, col, rc, fx.L.giql_hip_last_error())
        if new is None:         # the new plan is empty: its fill succeeds and writes nothing
            assert _untouched(outs), (row, col, "the fill of an empty plan wrote")
        else:
            assert np.array_equal(_result(row, outs, n), truth(*new)), (row, col, "the new plan's fill")
            assert _untouched([o[n:] for o in outs])


ORDERED_PAIRS = [(x, y) for x in ROWS for y in ROWS if x != y]


@pytest.mark.gpu
@pytest.mark.parametrize("made,other", ORDERED_PAIRS, ids=[f"{x}-then-fill-{y}" for x, y in ORDERED_PAIRS])
def test_a_plan_answers_only_its_own_fill(fx, made, other):
    """After each of the four plan calls the fill entry points of the other plans refuse: at most one plan is live.
    (INNER and the within-distance plan share ``giql_hip_inner_fill_dev``: of that pair, the later plan is the one it
    fills.)"""
    # a plan of the OTHER kind first: were the kinds kept side by side, it would still be there after `made`
    assert fx.plan(other)[0] == 0
    rc, n = fx.plan(made)
    assert (rc, n) == (0, truth(made, "a", "b").shape[0])
    rc, outs = fx.fill(other, 1 << 15)
    if {made, other} == {"INNER", "WINDOW"}:
        assert rc == 0 and np.array_equal(_result(made, outs, n), truth(made, "a", "b")), (made, other)
        assert not np.array_equal(truth(made, "a", "b"), truth(other, "a", "b"))
        return
    assert rc == fx.lib.GIQL_ERR_STATE and MESSAGES[other] in fx.L.giql_hip_last_error(), (made, other, rc)
    assert _untouched(outs), (made, other, "a refused fill wrote")
    rc, outs = fx.fill(made, n)
    assert rc == 0 and np.array_equal(_result(made, outs, n), truth(made, "a", "b")), (made, other, "its own fill")


# ---------------------------------------------------------------- export, on a plan that has a compact form
INNER_KEEPING = [col for col, words in TABLE.items() if words[0] == K]


@pytest.fixture(scope="module")
def fx_compact():
    """A context of its own: its INNER plans have only ever seen the fixed-length table."""
    f = Fixture()
    yield f, _columns(f)
    f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("col", INNER_KEEPING)
def test_export_of_a_compact_plan(fx_compact, col):
    """``kept`` for the export entry point: GIQL_OK, and the exported plan expands to the brute-force pairs."""
    from _plans import expand_np

    f, cols = fx_compact
    want = truth("INNER", "q", "u")
    assert f.plan("INNER", "q", "u") == (0, want.shape[0])
    status = cols[col]()
    refused = col in ("disjoin_fill", "contain_fill")           # the fills of the plans the context does not hold
    assert status == (f.lib.GIQL_ERR_STATE if refused else 0), (col, status, f.L.giql_hip_last_error())
    outs = [torch.full((512,), SENTINEL, dtype=torch.int32, device="cuda:0") for _ in range(4)]
    qia, nq, ns = ctypes.c_int32(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = f.L.giql_hip_inner_plan_export_dev(f.h, *(o.data_ptr() for o in outs), 512, 512, 0, 0, ctypes.byref(qia),
                                            ctypes.byref(nq), ctypes.byref(ns), f.st())
    assert rc == 0, (col, rc, f.L.giql_hip_last_error())
    assert {nq.value, ns.value} == {f.n["q"], f.n["u"]}
    q_rid, lo, cnt = (o[:nq.value].cpu().numpy() for o in outs[:3])
    s_rid = outs[3][:ns.value].cpu().numpy()
    row_q, row_s = expand_np(q_rid, lo.view(np.uint32), cnt.view(np.uint32), s_rid)
    got = ora.sort_pairs(row_q, row_s) if qia.value else ora.sort_pairs(row_s, row_q)
    assert np.array_equal(got, want), col
    assert _untouched([o[nq.value:] for o in outs[:3]] + [outs[3][ns.value:]])
    # and the fill beside it
    rc, filled = f.fill("INNER", want.shape[0])
    assert rc == 0 and np.array_equal(_result("INNER", filled, want.shape[0]), want), col
