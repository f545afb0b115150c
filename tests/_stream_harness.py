"""The stale / fresh protocol of tests/test_streams_gpu.py, its cases and their references.

A case is one call sequence on a ``HipEngine`` whose device inputs are rewritten, on a side stream ``s`` and behind a
bounded delay, from ``STALE`` to ``FRESH`` just before the call and back to ``STALE`` right after it.  Both sets are
valid inputs of the operator (same shapes, same row counts, same id ranges, same string bytes in all), so work that
runs out of stream order computes a wrong answer and never an out-of-range access.

The protocol speaks to the device through a small backend (``TorchBackend``); ``FakeBackend`` is a host model of
stream order -- work given to a side stream runs only when somebody waits for it -- on which the CPU tests show that
the protocol tells an entry point that launches on the caller's stream from one that launches on the null stream.
"""

from __future__ import annotations

import contextlib
import ctypes
import functools
import glob
import math
import os
import re
from dataclasses import dataclass

import numpy as np

from oracle import pyoracle as ora
from test_context_transitions import _rows

HERE = os.path.dirname(os.path.abspath(__file__))
STALE_SEED, FRESH_SEED = 7100, 7200


# ---------------------------------------------------------------------------------------------- backends
class TorchBackend:
    """The device: torch tensors on ``cuda:0``, ``torch.cuda.Stream`` streams."""

    def __init__(self):
        import torch

        self.torch = torch
        self.device = torch.device("cuda", 0)

    def upload(self, x):
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            return self.torch.from_numpy(np.ascontiguousarray(x)).to(self.device)

    def synchronize(self):
        self.torch.cuda.synchronize()

    def stream(self, s):
        return self.torch.cuda.stream(s)

    def sleep(self, cycles):
        self.torch.cuda._sleep(int(cycles))

    def copy(self, dst, src):
        dst.copy_(src, non_blocking=True)

    def clone(self, t):
        return t.clone()

    def to_host(self, tree):
        if isinstance(tree, self.torch.Tensor):
            return tree.cpu().numpy()
        if isinstance(tree, (tuple, list)):
            return tuple(self.to_host(t) for t in tree)
        return tree

    def stream_synchronize(self, s):
        s.synchronize()


class FakeTensor:
    def __init__(self, arr):
        self.arr = arr


class FakeStream:
    """Work in order; nothing of it runs before the host waits for the stream (or for the device)."""

    def __init__(self, be):
        self.queue = []
        be.streams.append(self)


class FakeBackend:
    """Stream order on the host.  The default stream runs its work at once; a side stream keeps it queued behind
    its delay until the host waits for that stream (a delay that outlasts every launch of the call: what the GPU
    tests calibrate).  ``log`` holds every step, in the order the host issued it."""

    def __init__(self):
        self.current = None          # None: the default stream
        self.streams = []
        self.log = []

    def _issue(self, what, fn, stream="current"):
        s = self.current if stream == "current" else stream
        self.log.append((what, "default" if s is None else "side"))
        if s is None:
            fn()
        else:
            s.queue.append(fn)

    def _drain(self, s):
        while s.queue:
            s.queue.pop(0)()

    def upload(self, x):
        self.log.append(("upload", "default" if self.current is None else "side"))
        return FakeTensor(np.array(x, copy=True))

    def synchronize(self):
        self.log.append(("synchronize", "device"))
        for s in self.streams:
            self._drain(s)

    @contextlib.contextmanager
    def stream(self, s):
        before, self.current = self.current, s
        try:
            yield
        finally:
            self.current = before

    def sleep(self, cycles):
        self._issue("sleep", lambda: None)

    def copy(self, dst, src):
        def run():
            dst.arr[...] = src.arr
        self._issue("copy", run)

    def clone(self, t):
        out = FakeTensor(np.empty_like(t.arr))

        def run():
            out.arr[...] = t.arr
        self._issue("clone", run)
        return out

    def launch(self, fn, null_stream=False):
        """What an entry point does: ``fn`` on the current stream, or (a mis-streamed one) on the null stream."""
        self._issue("launch", fn, stream=None if null_stream else "current")

    def to_host(self, tree):
        self.log.append(("to_host", "default" if self.current is None else "side"))
        if self.current is not None:
            self._drain(self.current)      # a blocking copy on the current stream waits for it
        return self._host(tree)

    def _host(self, tree):
        if isinstance(tree, FakeTensor):
            return tree.arr.copy()
        if isinstance(tree, (tuple, list)):
            return tuple(self._host(t) for t in tree)
        return tree

    def stream_synchronize(self, s):
        self.log.append(("stream_synchronize", "side"))
        self._drain(s)


# ---------------------------------------------------------------------------------------------- the protocol
def run_protocol(be, s, stale, fresh, call, delay_cycles):
    """Steps 1 to 7 for one call.  ``stale`` / ``fresh``: name -> numpy array; ``call(bufs)`` issues the operator on
    the current stream over the device buffers ``bufs`` (name -> tensor) and returns a tree of tensors and numbers.
    Returns ``(result on the host, {name: the buffer as the call left it, on the host})``."""
    assert sorted(stale) == sorted(fresh)
    for k in stale:
        assert stale[k].shape == fresh[k].shape and stale[k].dtype == fresh[k].dtype, k
    # 1. the buffers hold STALE, both staging sets are on the device, nothing is pending anywhere
    bufs = {k: be.upload(v) for k, v in stale.items()}
    staged_fresh = {k: be.upload(v) for k, v in fresh.items()}
    staged_stale = {k: be.upload(v) for k, v in stale.items()}
    be.synchronize()
    with be.stream(s):
        be.sleep(delay_cycles)                                     # 2.
        for k in bufs:                                             # 3. device-to-device, behind the delay
            be.copy(bufs[k], staged_fresh[k])
        out = call(bufs)                                           # 4.
        clones = {k: be.clone(bufs[k]) for k in bufs}              # 5. what the call left of its inputs
        for k in bufs:                                             # 6. the caller reuses the buffers, in stream order
            be.copy(bufs[k], staged_stale[k])
        host_out = be.to_host(out)                                 # 7.
        host_clones = {k: be.to_host(v) for k, v in clones.items()}
    be.stream_synchronize(s)     # every tensor above lived until here: no block went back to the allocator early
    del bufs, staged_fresh, staged_stale, clones, out
    return host_out, host_clones


def control_clones(be, s, stale, fresh, delay_cycles):
    """Control 1: steps 1 to 3, then one clone of every buffer issued under the default stream and one under ``s``.
    Returns ``(default-stream clones, side-stream clones)`` on the host."""
    bufs = {k: be.upload(v) for k, v in stale.items()}
    staged_fresh = {k: be.upload(v) for k, v in fresh.items()}
    be.synchronize()
    with be.stream(s):
        be.sleep(delay_cycles)
        for k in bufs:
            be.copy(bufs[k], staged_fresh[k])
    early = {k: be.clone(bufs[k]) for k in bufs}           # the default stream: nothing orders it behind s
    host_early = {k: be.to_host(v) for k, v in early.items()}
    with be.stream(s):
        late = {k: be.clone(bufs[k]) for k in bufs}
        host_late = {k: be.to_host(v) for k, v in late.items()}
    be.stream_synchronize(s)
    del bufs, staged_fresh, early, late
    return host_early, host_late


# ---------------------------------------------------------------------------------------------- comparing trees
class Approx:
    """A reference value with a derived error bound per element."""

    def __init__(self, want, bound):
        self.want, self.bound = np.asarray(want, np.float64), np.asarray(bound, np.float64)


def same(got, want) -> bool:
    if isinstance(want, Approx):
        got = np.asarray(got, np.float64)
        return got.shape == want.want.shape and bool(np.all(np.abs(got - want.want) <= want.bound))
    if isinstance(want, (tuple, list)):
        return isinstance(got, (tuple, list)) and len(got) == len(want) and all(same(g, w) for g, w in zip(got, want))
    if isinstance(want, np.ndarray):
        got = np.asarray(got)
        if got.shape != want.shape:
            return False
        if want.dtype.kind in "fc":
            return got.dtype == want.dtype and got.tobytes() == want.tobytes()
        return bool(np.array_equal(got, want))
    return got == want


def exact_part(tree):
    """The tree without its ``Approx`` leaves (their reference values stand in): what two references are told apart by."""
    if isinstance(tree, Approx):
        return tree.want
    if isinstance(tree, (tuple, list)):
        return tuple(exact_part(t) for t in tree)
    return tree


def bitwise_equal(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------- inputs
RECIPE_CHROMS = {"general": 4, "uniform_b": 4, "presorted": 4, "pileups": 2}


def _put(out, prefix, side):
    out[prefix + ".chrom"], out[prefix + ".start"], out[prefix + ".end"] = side.chrom, side.start, side.end


def two_tables(recipe, na=3000, nb=20_000):
    """The recipe of ``test_context_transitions._build_classes`` of that name, by seed: ~3,000 x ~20,000 rows."""
    nch = RECIPE_CHROMS[recipe]

    def make(seed):
        r = np.random.default_rng(seed)
        if recipe == "pileups":
            a = _rows(r, na, nch, 4_000_000, (1, 2000))
            b = _rows(r, nb, nch, 4_000_000, (1, 3000))
            b.start[:] = (r.integers(0, 200, b.n) * 20_000).astype(np.int32)
            b.end[:] = b.start + r.integers(1, 3000, b.n).astype(np.int32)
        else:
            a = _rows(r, na, nch, 8_000_000, (1, 2000))
            b = _rows(r, nb, nch, 8_000_000, 150 if recipe == "uniform_b" else (1, 800))
            if recipe == "presorted":
                sa, sb = np.lexsort((a.start, a.chrom)), np.lexsort((b.start, b.chrom))
                a, b = ora.Side(a.chrom[sa], a.start[sa], a.end[sa]), ora.Side(b.chrom[sb], b.start[sb], b.end[sb])
        out = {}
        _put(out, "a", a)
        _put(out, "b", b)
        return out

    return make


def one_table(n=5000, nch=5):
    def make(seed):
        r = np.random.default_rng(seed)
        out = {}
        _put(out, "a", _rows(r, n, nch, 100_000, (1, 60)))
        return out

    return make


def hside(inp, prefix, offs=(0, 0)):
    return ora.Side(inp[prefix + ".chrom"], inp[prefix + ".start"], inp[prefix + ".end"], *offs)


def dside(bufs, prefix, offs=(0, 0)):
    from giql_amd.engine import DeviceSide

    return DeviceSide(bufs[prefix + ".chrom"], bufs[prefix + ".start"], bufs[prefix + ".end"], *offs)


def _with(make, extra):
    """``make`` plus the arrays ``extra(rng, inputs)`` adds."""
    def both(seed):
        out = make(seed)
        out.update(extra(np.random.default_rng(seed + 50_000), out))
        return out

    return both


def utf8_column(r, lengths):
    """Arrow utf8 buffers of one string per entry of ``lengths``, in an order the seed picks: ``(offsets int32,
    data uint8)``.  Every seed gives the same number of rows and of bytes."""
    lengths = np.asarray(lengths, np.int64)[r.permutation(len(lengths))]
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    data = r.integers(97, 123, int(off[-1])).astype(np.uint8)
    return off, data


def utf8_rows(off, data):
    raw = np.asarray(data, np.uint8).tobytes()
    return [raw[off[i]:off[i + 1]] for i in range(len(off) - 1)]


# ---------------------------------------------------------------------------------------------- references
def sort_pairs(ra, rb):
    p = np.stack([np.asarray(ra, np.int64), np.asarray(rb, np.int64)], 1)
    return p[np.lexsort((p[:, 1], p[:, 0]))]


def pairs_where(a, b, pred):
    """Sorted ``[k, 2]`` pairs of rows on one chromosome for which ``pred(a.cs, a.ce, b.cs, b.ce)`` holds: the
    boolean matrix, one chromosome at a time."""
    out = [np.zeros((0, 2), np.int64)]
    for c in np.unique(a.chrom):
        ia, ib = np.nonzero(a.chrom == c)[0], np.nonzero(b.chrom == c)[0]
        if ia.size == 0 or ib.size == 0:
            continue
        acs, ace = a.cs[ia].astype(np.int64)[:, None], a.ce[ia].astype(np.int64)[:, None]
        bcs, bce = b.cs[ib].astype(np.int64)[None, :], b.ce[ib].astype(np.int64)[None, :]
        r, k = np.nonzero(pred(acs, ace, bcs, bce))
        out.append(np.stack([ia[r], ib[k]], 1).astype(np.int64))
    p = np.concatenate(out)
    return p[np.lexsort((p[:, 1], p[:, 0]))]


def contains(acs, ace, bcs, bce):
    return (acs <= bcs) & (ace >= bce)


def within(acs, ace, bcs, bce):
    return (bcs <= acs) & (bce >= ace)


def within_distance(n):
    return lambda acs, ace, bcs, bce: (acs - n < bce) & (ace + n > bcs)


def per_row(pairs, n_a):
    counts = np.bincount(pairs[:, 0], minlength=n_a).astype(np.int64)
    ids = np.arange(n_a, dtype=np.int64)
    return ids[counts > 0], ids[counts == 0], counts


def inner_pairs(inp, a="a", b="b"):
    return sort_pairs(*ora.c_inner(hside(inp, a), hside(inp, b), "sweep"))


def matched(b, idx, dist):
    """NEAREST rows as the operator's tests compare them: the distance and the (start, end) of the matched row."""
    idx, dist = np.asarray(idx, np.int64), np.asarray(dist, np.int64)
    none = idx < 0
    safe = np.where(none, 0, idx)
    return (none, np.where(none, 0, dist), np.where(none, -1, b.start[safe]), np.where(none, -1, b.end[safe]))


# ---------------------------------------------------------------------------------------------- the cases
@dataclass
class Case:
    id: str
    symbols: tuple                 # the entry points (giql_hip_<name>) the call sequence reaches
    make: object                   # seed -> {name: numpy array}
    ref: object                    # host inputs -> canonical tree (may hold Approx leaves)
    run: object                    # (engine, device buffers, prepared) -> tree of tensors and numbers
    canon: object = None           # (host result, FRESH host inputs) -> canonical tree
    engine: str = "default"        # "default": SideChain forks where the operator has one; "local": it never does
    prepare: object = None         # engine -> whatever the case builds once, before the protocol (an index)
    exempt: tuple = ()             # inputs the call may write (none so far: STRING_AGG's n_bytes is a host field)
    sidechain: bool = False        # the operator forks the context's second stream on the default engine

    def inputs(self, which):
        return _inputs(self.id, which)

    def want(self, which="fresh"):
        return _want(self.id, which)


CASES: dict = {}


def case(**kw):
    c = Case(**kw)
    assert c.id not in CASES, c.id
    CASES[c.id] = c
    return c


@functools.lru_cache(maxsize=None)
def _inputs(cid, which):
    out = CASES[cid].make({"stale": STALE_SEED, "fresh": FRESH_SEED}[which])
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _want(cid, which):
    return CASES[cid].ref(_inputs(cid, which))


def _identity(out, _inp):
    return out


def _pairs_canon(out, _inp):
    return sort_pairs(out[0], out[1])


# ---- INNER
def _plan_fill(eng, bufs, nch):
    import torch

    a, b = dside(bufs, "a"), dside(bufs, "b")
    n = eng.inner_plan(a, b, nch)
    ra = torch.empty(n, dtype=torch.int32, device=eng.device)
    rb = torch.empty(n, dtype=torch.int32, device=eng.device)
    eng.inner_fill(ra, rb)       # returns with the fill in flight: step 6 overwrites the inputs behind it
    return ra, rb


GUARD = 64


def _join_into(eng, bufs, nch, cap):
    import torch

    ra = torch.full((cap + GUARD,), -7, dtype=torch.int32, device=eng.device)
    rb = torch.full((cap + GUARD,), -7, dtype=torch.int32, device=eng.device)
    n = eng.inner_join_into(dside(bufs, "a"), dside(bufs, "b"), nch, ra[:cap], rb[:cap])
    return n, ra, rb


def _into_canon(out, _inp):
    n, ra, rb = out
    tail_clean = bool(np.all(ra[n:] == -7) and np.all(rb[n:] == -7))
    return n, tail_clean, sort_pairs(ra[:n], rb[:n])


def _into_ref(inp):
    p = inner_pairs(inp)
    return p.shape[0], True, p


def _into_cap(cid):
    """Room for the larger of the two results: a call that read STALE rows fails on its pairs, not on its capacity."""
    return max(_want(cid, "stale")[0], _want(cid, "fresh")[0])


for _recipe in ("general", "uniform_b", "presorted", "pileups"):
    _nch = RECIPE_CHROMS[_recipe]
    case(id=f"inner_join[{_recipe}]", symbols=("inner_plan", "inner_fill", "inner_join"), make=two_tables(_recipe),
         ref=inner_pairs, canon=_pairs_canon, sidechain=True,
         run=lambda eng, bufs, _p, nch=_nch: eng.inner_join(dside(bufs, "a"), dside(bufs, "b"), nch))
case(id="inner_join[general]@local", symbols=("inner_plan", "inner_fill", "inner_join"), make=two_tables("general"),
     ref=inner_pairs, canon=_pairs_canon, engine="local",
     run=lambda eng, bufs, _p: eng.inner_join(dside(bufs, "a"), dside(bufs, "b"), 4))
case(id="inner_plan_fill[general]", symbols=("inner_plan", "inner_fill"), make=two_tables("general"),
     ref=inner_pairs, canon=_pairs_canon, sidechain=True, run=lambda eng, bufs, _p: _plan_fill(eng, bufs, 4))
case(id="inner_plan_fill[uniform_b]", symbols=("inner_plan", "inner_fill"), make=two_tables("uniform_b"),
     ref=inner_pairs, canon=_pairs_canon, sidechain=True, run=lambda eng, bufs, _p: _plan_fill(eng, bufs, 4))
for _recipe in ("general", "uniform_b"):
    case(id=f"inner_join_into[{_recipe}]", symbols=("inner_join",), make=two_tables(_recipe), ref=_into_ref,
         canon=_into_canon, sidechain=True,
         run=lambda eng, bufs, _p, cid=f"inner_join_into[{_recipe}]": _join_into(eng, bufs, 4, _into_cap(cid)))


def _export_run(eng, bufs, _p):
    import torch

    a, b = dside(bufs, "a"), dside(bufs, "b")
    n = eng.inner_plan(a, b, 4)
    i32 = dict(dtype=torch.int32, device=eng.device)
    q_rid, lo, cnt = (torch.full((a.n,), -7, **i32) for _ in range(3))
    s_rid = torch.full((b.n,), -7, **i32)
    sizes = eng.plan_export(q_rid, lo, cnt, s_rid)
    return n, sizes, q_rid, lo, cnt, s_rid


def _export_canon(out, inp):
    from _plans import expand_np

    n, (q_is_a, n_q, n_s), q_rid, lo, cnt, s_rid = out
    na, nb = inp["a.chrom"].shape[0], inp["b.chrom"].shape[0]
    if (q_is_a, n_q, n_s) != (True, na, nb) or lo.min() < 0 or cnt.min() < 0 or (lo.astype(np.int64) + cnt).max() > n_s:
        return ("no plan of the query side A", q_is_a, n_q, n_s)
    rq, rs = expand_np(q_rid, lo, cnt, s_rid)
    return n, sort_pairs(rq, rs)


def _export_ref(inp):
    p = inner_pairs(inp)
    return p.shape[0], p


case(id="plan_export[uniform_b]", symbols=("inner_plan", "inner_plan_export"), make=two_tables("uniform_b"),
     ref=_export_ref, canon=_export_canon, run=_export_run, sidechain=True)

PLAN_NQ, PLAN_NS, PLAN_MAX_CNT = 10_000, 4000, 8


def _plan_make(seed):
    """A compact plan whose every row keeps ``lo + PLAN_MAX_CNT <= n_s``: any mix of two such plans stays in range."""
    r = np.random.default_rng(seed)
    return {"q_rid": r.permutation(PLAN_NQ).astype(np.int32) + 7_000_000,
            "lo": r.integers(0, PLAN_NS - PLAN_MAX_CNT + 1, PLAN_NQ).astype(np.int32),
            "cnt": r.integers(0, PLAN_MAX_CNT, PLAN_NQ).astype(np.int32),
            "s_rid": r.permutation(PLAN_NS).astype(np.int32) + 1_000_000}


def _plan_run(eng, bufs, _p):
    import torch

    cap = PLAN_NQ * PLAN_MAX_CNT       # room for every plan of these shapes
    rq = torch.full((cap + GUARD,), -7, dtype=torch.int32, device=eng.device)
    rs = torch.full((cap + GUARD,), -7, dtype=torch.int32, device=eng.device)
    n = eng.fill_from_plan(bufs["q_rid"], bufs["lo"], bufs["cnt"], bufs["s_rid"], rq[:cap], rs[:cap])
    return n, rq, rs


def _plan_canon(out, _inp):
    n, rq, rs = out
    return n, bool(np.all(rq[n:] == -7) and np.all(rs[n:] == -7)), rq[:n].copy(), rs[:n].copy()


def _plan_ref(inp):
    from _plans import expand_np

    rq, rs = expand_np(inp["q_rid"], inp["lo"], inp["cnt"], inp["s_rid"])
    return rq.shape[0], True, rq.astype(np.int32), rs.astype(np.int32)


case(id="fill_from_plan", symbols=("fill_from_plan",), make=_plan_make, ref=_plan_ref, canon=_plan_canon, run=_plan_run)


def _miss_make(seed):
    u, g = two_tables("uniform_b")(seed), two_tables("general")(seed + 1)
    return {**{"u." + k: v for k, v in u.items()}, **{"g." + k: v for k, v in g.items()}}


def _miss_run(eng, bufs, _p):
    first = eng.inner_join(dside(bufs, "u.a"), dside(bufs, "u.b"), 4)
    form_u = eng.stats()["join_form"]
    # the context now speculates on a fixed-length B: this call's read-back shows the miss and the call repeats itself
    second = eng.inner_join(dside(bufs, "g.a"), dside(bufs, "g.b"), 4)
    return first, form_u, second, eng.stats()["join_form"]


case(id="inner_join[guess_miss]", symbols=("inner_plan", "inner_fill", "inner_join"), make=_miss_make, sidechain=True,
     ref=lambda inp: (inner_pairs(inp, "u.a", "u.b"), "uniform_b", inner_pairs(inp, "g.a", "g.b"), "general"),
     canon=lambda out, _inp: (sort_pairs(*out[0]), out[1], sort_pairs(*out[2]), out[3]), run=_miss_run)

# ---- SEMI / ANTI / COUNT
for _eng in ("default", "local"):
    _sfx = "" if _eng == "default" else "@local"
    case(id="semi_join" + _sfx, symbols=("semi_anti",), make=two_tables("general"), engine=_eng, sidechain=_eng == "default",
         ref=lambda inp: np.asarray(ora.c_semi_anti(hside(inp, "a"), hside(inp, "b"), False)), canon=_identity,
         run=lambda eng, bufs, _p: eng.semi_join(dside(bufs, "a"), dside(bufs, "b"), 4))
    case(id="count_overlaps" + _sfx, symbols=("count",), make=two_tables("general"), engine=_eng, sidechain=_eng == "default",
         ref=lambda inp: np.asarray(ora.c_count(hside(inp, "a"), hside(inp, "b"), "sweep")), canon=_identity,
         run=lambda eng, bufs, _p: eng.count_overlaps(dside(bufs, "a"), dside(bufs, "b"), 4))
case(id="anti_join", symbols=("semi_anti",), make=two_tables("uniform_b"), sidechain=True,
     ref=lambda inp: np.asarray(ora.c_semi_anti(hside(inp, "a"), hside(inp, "b"), True)), canon=_identity,
     run=lambda eng, bufs, _p: eng.anti_join(dside(bufs, "a"), dside(bufs, "b"), 4))

ROW_PREDS = {"contains": (contains, None), "within": (within, None), "within_distance": (within_distance(1000), 1000)}
for _name, (_pred, _md) in ROW_PREDS.items():
    case(id=f"semi_anti_pred[{_name}]", symbols=("semi_anti_pred",), make=two_tables("general"),
         ref=lambda inp, pred=_pred: per_row(pairs_where(hside(inp, "a"), hside(inp, "b"), pred), inp["a.chrom"].shape[0])[:2],
         canon=_identity,
         run=lambda eng, bufs, _p, name=_name, md=_md: tuple(
             eng.semi_anti_pred(dside(bufs, "a"), dside(bufs, "b"), 4, name, anti, md) for anti in (False, True)))
    case(id=f"count_pred[{_name}]", symbols=("count_pred",), make=two_tables("general"),
         ref=lambda inp, pred=_pred: per_row(pairs_where(hside(inp, "a"), hside(inp, "b"), pred), inp["a.chrom"].shape[0])[2],
         canon=_identity,
         run=lambda eng, bufs, _p, name=_name, md=_md: eng.count_pred(dside(bufs, "a"), dside(bufs, "b"), 4, name, md))


# ---- NEAREST
def _nearest_case(cid, recipe, signed=False, md=None, engine="default"):
    nch = RECIPE_CHROMS[recipe]
    case(id=cid, symbols=("nearest",), make=two_tables(recipe), engine=engine, sidechain=engine == "default",
         ref=lambda inp: matched(hside(inp, "b"), *ora.c_nearest_k1(hside(inp, "a"), hside(inp, "b"), signed=signed,
                                                                       max_distance=md, method="sweep")),
         canon=lambda out, inp: matched(hside(inp, "b"), out[0], out[1]),
         run=lambda eng, bufs, _p: eng.nearest(dside(bufs, "a"), dside(bufs, "b"), nch, signed=signed, max_distance=md))


_nearest_case("nearest[signed]", "general", signed=True)
_nearest_case("nearest[max_distance]", "general", md=500)
_nearest_case("nearest[pileups]", "pileups")
_nearest_case("nearest@local", "general", engine="local")
case(id="nearest32", symbols=("nearest32",), make=two_tables("general"), sidechain=True,
     ref=lambda inp: matched(hside(inp, "b"), *ora.c_nearest_k1(hside(inp, "a"), hside(inp, "b"), method="sweep")),
     canon=lambda out, inp: matched(hside(inp, "b"), out[:, 0], out[:, 1]),
     run=lambda eng, bufs, _p: eng.nearest32(dside(bufs, "a"), dside(bufs, "b"), 4))


def _nearest_k_case(cid, recipe, k):
    nch = RECIPE_CHROMS[recipe]
    case(id=cid, symbols=("nearest_k",), make=two_tables(recipe),
         ref=lambda inp: matched(hside(inp, "b"), *ora.c_nearest_k(hside(inp, "a"), hside(inp, "b"), k)),
         canon=lambda out, inp: matched(hside(inp, "b"), out[0], out[1]),
         run=lambda eng, bufs, _p: eng.nearest_k(dside(bufs, "a"), dside(bufs, "b"), nch, k))


_nearest_k_case("nearest_k[3]", "general", 3)          # the records path
_nearest_k_case("nearest_k[17]", "general", 17)        # the direct path
_nearest_k_case("nearest_k[3,pileups]", "pileups", 3)  # the two-sort repeat


# ---- one table: CLUSTER / MERGE / aggregates / GROUP BY / DISJOIN
def _payload(r, inp):
    m = inp["a.chrom"].shape[0]
    col = np.repeat(r.integers(0, 3, m // 40 + 1), 40)[:m].astype(np.int32)[r.permutation(m)]
    return {"col": col, "col.valid": (r.random(m) > 0.05).astype(np.uint8)}


def _holds(inp):
    col, valid = inp["col"], inp["col.valid"]
    return lambda i, j: bool(valid[i]) and bool(valid[j]) and col[i] == col[j]


def _cluster_pred_ids(inp, distance):
    return ora.py_cluster_predicate(inp["a.chrom"].tolist(), inp["a.start"].tolist(), inp["a.end"].tolist(), distance,
                                    _holds(inp))


def _regions_of_ids(inp, ids):
    regions = {}
    for c, cid, st, en in zip(inp["a.chrom"].tolist(), np.asarray(ids).tolist(), inp["a.start"].tolist(),
                              inp["a.end"].tolist()):
        g = regions.setdefault((c, cid), [st, en, 0])
        g[0], g[1], g[2] = min(g[0], st), max(g[1], en), g[2] + 1
    return np.array(sorted((c, g[0], g[1], g[2]) for (c, _), g in regions.items()), np.int64)


def _preds(bufs):
    return [(("a", bufs["col"], bufs["col.valid"]), "=", ("b", bufs["col"], bufs["col.valid"]))]


DIST = 40
case(id="cluster", symbols=("cluster",), make=one_table(), canon=_identity,
     ref=lambda inp: np.asarray(ora.c_cluster(hside(inp, "a"), DIST)),
     run=lambda eng, bufs, _p: eng.cluster(dside(bufs, "a"), 5, DIST))
case(id="cluster[preds]", symbols=("cluster_pred",), make=_with(one_table(), _payload), canon=_identity,
     ref=lambda inp: np.asarray(_cluster_pred_ids(inp, DIST), np.int64),
     run=lambda eng, bufs, _p: eng.cluster(dside(bufs, "a"), 5, DIST, preds=_preds(bufs)))
case(id="merge", symbols=("merge",), make=one_table(),
     ref=lambda inp: np.stack([np.asarray(x, np.int64) for x in ora.c_merge(hside(inp, "a"), DIST)], 1),
     canon=lambda out, _inp: np.stack([np.asarray(x, np.int64) for x in out], 1),
     run=lambda eng, bufs, _p: eng.merge(dside(bufs, "a"), 5, DIST))
case(id="merge[preds]", symbols=("merge_pred",), make=_with(one_table(), _payload),
     ref=lambda inp: _regions_of_ids(inp, _cluster_pred_ids(inp, DIST)),
     # (regions of one chromosome that start on one position have no order among them: compared as a sorted list)
     canon=lambda out, _inp: np.array(sorted(zip(*(np.asarray(x, np.int64).tolist() for x in out))), np.int64).reshape(-1, 4),
     run=lambda eng, bufs, _p: eng.merge(dside(bufs, "a"), 5, DIST, preds=_preds(bufs)))

AGG_FUNCS = ("SUM", "AVG", "MIN", "MAX")


def _agg_columns(r, inp):
    n = inp["a.chrom"].shape[0]
    return {"vi": r.integers(-1_000_000, 1_000_000, n).astype(np.int64), "vi.valid": (r.random(n) >= 0.3).astype(np.uint8),
            "vf": (r.normal(0, 1000, n) * r.choice([1e-3, 1.0, 1e3], n)).astype(np.float64),
            "vf.valid": (r.random(n) >= 0.3).astype(np.uint8)}


def _agg_ref(inp, distance=DIST):
    """MERGE's four columns, then per aggregate ``(values, valid)``: exact but for float SUM / AVG, which carry the
    bound of tests/test_merge_aggregates_gpu.py -- k * 2^-52 * sum|x| for a SUM of k values, that over k plus one ulp
    of the result for an AVG."""
    import _merge_agg_ref as R

    regions = R.regions(inp["a.chrom"].tolist(), inp["a.start"].tolist(), inp["a.end"].tolist(), distance)
    start, end = inp["a.start"], inp["a.end"]
    head = np.array([[p, min(int(start[i]) for i in m), max(int(end[i]) for i in m), len(m)] for p, m in regions], np.int64)
    out = [head]
    for name in ("vi", "vf"):
        if name not in inp:
            continue
        flt = inp[name].dtype.kind == "f"
        py = [v.item() if ok else None for v, ok in zip(inp[name], inp[name + ".valid"])]
        for func in AGG_FUNCS:
            vals, bounds, valid = [], [], []
            for _p, members in regions:
                xs = [py[i] for i in members]
                want = R.aggregate(func, xs)
                valid.append(want is not None)
                vals.append(0 if want is None else want)
                k = sum(x is not None for x in xs)
                bound = 0.0
                if want is not None and flt and func in ("SUM", "AVG"):
                    bound = k * 2.0 ** -52 * R.abs_sum(xs)
                    bound = bound if func == "SUM" else bound / k + math.ulp(want)
                bounds.append(bound)
            as_float = flt or func == "AVG"
            values = Approx(vals, bounds) if as_float else np.array(vals, np.int64)
            out.append((values, np.array(valid, bool)))
    return tuple(out)


def _agg_entries(bufs):
    return [(f, bufs[name], bufs[name + ".valid"]) for name in ("vi", "vf") for f in AGG_FUNCS]


def _agg_canon(out, _inp):
    head = np.stack([np.asarray(x, np.int64) for x in out[:4]], 1)
    return (head,) + tuple((np.asarray(v), np.asarray(ok, bool)) for v, ok in out[4:])


case(id="merge_agg", symbols=("merge_agg",), make=_with(one_table(), _agg_columns), ref=_agg_ref, canon=_agg_canon,
     run=lambda eng, bufs, _p: eng.merge_agg(dside(bufs, "a"), 5, DIST, _agg_entries(bufs)))

STR_LENGTHS = [0, 1, 3, 5, 8, 12, 31, 32, 33, 2] * 500     # 5,000 rows


def _str_columns(r, inp):
    off, data = utf8_column(r, STR_LENGTHS)
    n = inp["a.chrom"].shape[0]
    return {"w.off": off, "w.data": data, "w.valid": (r.random(n) >= 0.2).astype(np.uint8),
            "vi": r.integers(-1000, 1000, n).astype(np.int64), "vi.valid": (r.random(n) >= 0.3).astype(np.uint8)}


def _str_ref(inp):
    import _merge_agg_ref as R
    from _string_agg_ref import members_in_order

    regions = R.regions(inp["a.chrom"].tolist(), inp["a.start"].tolist(), inp["a.end"].tolist(), DIST)
    start, end = inp["a.start"], inp["a.end"]
    head = np.array([[p, min(int(start[i]) for i in m), max(int(end[i]) for i in m), len(m)] for p, m in regions], np.int64)
    words, ok = utf8_rows(inp["w.off"], inp["w.data"]), inp["w.valid"]
    joined = []
    for _p, members in regions:
        vals = [words[i] for i in members_in_order(members, start) if ok[i]]
        joined.append(b";".join(vals) if vals else None)
    vi = [v.item() if k else None for v, k in zip(inp["vi"], inp["vi.valid"])]
    sums = [R.aggregate("SUM", [vi[i] for i in m]) for _p, m in regions]
    return head, tuple(joined), (np.array([0 if s is None else s for s in sums], np.int64),
                                 np.array([s is not None for s in sums], bool))


def _str_canon(out, _inp):
    head = np.stack([np.asarray(x, np.int64) for x in out[:4]], 1)
    off, data, ok = out[4]
    rows = utf8_rows(off, data)
    return head, tuple(r if k else None for r, k in zip(rows, ok)), (np.asarray(out[5][0]), np.asarray(out[5][1], bool))


case(id="merge_agg[STRING_AGG]", symbols=("merge_str", "concat_utf8_fill"), make=_with(one_table(), _str_columns),
     ref=_str_ref, canon=_str_canon,
     run=lambda eng, bufs, _p: eng.merge_agg(dside(bufs, "a"), 5, DIST, [
         ("STRING_AGG", bufs["w.off"], bufs["w.data"], bufs["w.valid"], ";"), ("SUM", bufs["vi"], bufs["vi.valid"])]))


def _group_make(seed):
    r = np.random.default_rng(seed)
    s0 = _rows(r, 3000, 5, 100_000, (1, 60))
    pick = np.concatenate([np.arange(s0.n), r.integers(0, s0.n, 2000)])[r.permutation(5000)]    # duplicate keys
    out = {"vals": r.integers(-2**40, 2**40, 5000).astype(np.int64)}
    _put(out, "a", ora.Side(s0.chrom[pick], s0.start[pick], s0.end[pick]))
    return out


def _group_ref(inp):
    keys = np.stack([inp["a.chrom"], inp["a.start"], inp["a.end"]], 1).astype(np.int64)
    uniq, inv = np.unique(keys, axis=0, return_inverse=True)
    sums = np.zeros(uniq.shape[0], np.int64)
    np.add.at(sums, inv.reshape(-1), inp["vals"])
    return inv.reshape(-1).astype(np.int64), uniq, sums


def _group_run(eng, bufs, _p):
    gid, rep = eng.group_rows(dside(bufs, "a"), 5)
    return gid, rep, eng.segment_sum(bufs["vals"], gid, int(rep.shape[0]))


def _group_canon(out, inp):
    gid, rep, sums = out
    keys = np.stack([inp["a.chrom"], inp["a.start"], inp["a.end"]], 1).astype(np.int64)
    return gid.astype(np.int64), keys[rep], sums


case(id="group_rows+segment_sum", symbols=("group_rows", "segment_sum"), make=_group_make, ref=_group_ref,
     canon=_group_canon, run=_group_run)

SEG_GROUPS = 700


def _seg_ref(inp):
    sums = np.zeros(SEG_GROUPS, np.int64)
    np.add.at(sums, inp["gid"], inp["vals"])
    return sums


case(id="segment_sum", symbols=("segment_sum",), canon=_identity, ref=_seg_ref,
     make=lambda seed: {"vals": np.random.default_rng(seed).integers(-2**40, 2**40, 10_000).astype(np.int64),
                        "gid": np.random.default_rng(seed + 1).integers(0, SEG_GROUPS, 10_000).astype(np.int32)},
     run=lambda eng, bufs, _p: eng.segment_sum(bufs["vals"], bufs["gid"], SEG_GROUPS))


def _disjoin_ref(inp, mode):
    from _disjoin_ref import brute_force_arrays

    i64 = lambda p: [inp[p + ".chrom"].astype(np.int64), inp[p + ".start"].astype(np.int64), inp[p + ".end"].astype(np.int64)]
    return brute_force_arrays(*i64("a")) if mode == "self" else brute_force_arrays(*i64("a"), *i64("b"))


def _disjoin_canon(out, _inp):
    return np.stack([np.asarray(x, np.int64) for x in out], 1)


case(id="disjoin[self]", symbols=("disjoin_plan", "disjoin_fill"), make=two_tables("general"), canon=_disjoin_canon,
     ref=lambda inp: _disjoin_ref(inp, "self"), run=lambda eng, bufs, _p: eng.disjoin(dside(bufs, "a"), None, 4))
case(id="disjoin[reference]", symbols=("disjoin_plan", "disjoin_fill"), make=two_tables("general"), canon=_disjoin_canon,
     ref=lambda inp: _disjoin_ref(inp, "reference"),
     run=lambda eng, bufs, _p: eng.disjoin(dside(bufs, "a"), dside(bufs, "b"), 4))


# ---- coverage: DISJOIN's front (spans, events, one sort, two flag scans) and its own breakpoint rows, in one call
def _coverage_ref(inp, runs=False, with_depth=True):
    from _coverage_ref import sweep_arrays

    rows = sweep_arrays(inp["a.chrom"], inp["a.start"], inp["a.end"], runs=runs)
    return rows if with_depth else rows[:, :3].copy()


def _coverage_canon(out, _inp):
    return np.stack([np.asarray(x, np.int64) for x in out if x is not None], 1)


case(id="coverage[depth]", symbols=("coverage",), make=one_table(), ref=_coverage_ref, canon=_coverage_canon,
     run=lambda eng, bufs, _p: eng.coverage(dside(bufs, "a"), 5))
case(id="coverage[runs]", symbols=("coverage",), make=one_table(), canon=_coverage_canon,
     ref=lambda inp: _coverage_ref(inp, runs=True), run=lambda eng, bufs, _p: eng.coverage(dside(bufs, "a"), 5, runs=True))
case(id="coverage[distinct]", symbols=("coverage",), make=one_table(), canon=_coverage_canon,
     ref=lambda inp: _coverage_ref(inp, with_depth=False),
     run=lambda eng, bufs, _p: eng.coverage(dside(bufs, "a"), 5, with_depth=False))

# ---- the other joins
case(id="contain_join[a contains b]", symbols=("contain_plan", "contain_fill"), make=two_tables("general"),
     ref=lambda inp: pairs_where(hside(inp, "a"), hside(inp, "b"), contains), canon=_pairs_canon,
     run=lambda eng, bufs, _p: eng.contain_join(dside(bufs, "a"), dside(bufs, "b"), 4))
case(id="contain_join[b contains a]", symbols=("contain_plan", "contain_fill"), make=two_tables("general"),
     ref=lambda inp: pairs_where(hside(inp, "b"), hside(inp, "a"), contains), canon=_pairs_canon,
     run=lambda eng, bufs, _p: eng.contain_join(dside(bufs, "b"), dside(bufs, "a"), 4))


def _strands(r, inp):
    return {"a.strand": r.integers(0, 5, inp["a.chrom"].shape[0]).astype(np.int32),
            "b.strand": r.integers(0, 5, inp["b.chrom"].shape[0]).astype(np.int32)}


def _window_run(eng, bufs, _p):
    a, b = dside(bufs, "a"), dside(bufs, "b")
    ra, rb = eng.window_join(a, b, 4, 1000)
    signed = eng.distance(a, b, ra, rb, signed=True)
    stranded = eng.distance(a, b, ra, rb, signed=True, stranded=True, strand_a=bufs["a.strand"], strand_b=bufs["b.strand"])
    return ra, rb, signed, stranded


def _window_canon(out, _inp):
    ra, rb, (d1, v1), (d2, v2) = out
    o = np.lexsort((rb, ra))
    v1, v2 = v1[o] != 0, v2[o] != 0
    return (np.stack([ra[o], rb[o]], 1).astype(np.int64), np.where(v1, d1[o], 0), v1, np.where(v2, d2[o], 0), v2)


def _window_ref(inp):
    import _distance_ref as D

    a, b = hside(inp, "a"), hside(inp, "b")
    p = pairs_where(a, b, within_distance(1000))
    ra, rb = p[:, 0], p[:, 1]
    cols = (a.chrom[ra], a.cs[ra], a.ce[ra], b.chrom[rb], b.cs[rb], b.ce[rb])
    d1, v1 = D.distance(*cols, signed=True)
    d2, v2 = D.distance(*cols, signed=True, stranded=True, strand_a=inp["a.strand"][ra], strand_b=inp["b.strand"][rb])
    v1, v2 = np.asarray(v1, bool), np.asarray(v2, bool)
    return p, np.where(v1, d1, 0).astype(np.int64), v1, np.where(v2, d2, 0).astype(np.int64), v2


case(id="window_join+distance", symbols=("window_plan", "inner_fill", "distance"), make=_with(two_tables("general"), _strands),
     ref=_window_ref, canon=_window_canon, run=_window_run)


def _left_ref(inp):
    import _left_ref as L

    return L.left_rows(hside(inp, "a"), hside(inp, "b"))


def _left_canon(out, _inp):
    import _left_ref as L

    return L.sort_rows(out[0], out[1])


case(id="left_join", symbols=("inner_plan", "inner_fill", "inner_join", "left_pad"), make=two_tables("general"),
     ref=_left_ref, canon=_left_canon, sidechain=True,
     run=lambda eng, bufs, _p: eng.left_join(dside(bufs, "a"), dside(bufs, "b"), 4))

PAD_ROWS = 5000


def _pad_make(seed):
    r = np.random.default_rng(seed)
    return {"ra": r.integers(0, PAD_ROWS, 10_000).astype(np.int32) // 3 * 3,      # two rows in three have no pair
            "rb": r.integers(0, 20_000, 10_000).astype(np.int32)}


def _pad_ref(inp):
    pad = np.setdiff1d(np.arange(PAD_ROWS, dtype=np.int64), inp["ra"].astype(np.int64))
    return (np.concatenate([inp["ra"].astype(np.int64), pad]),
            np.concatenate([inp["rb"].astype(np.int64), np.full(pad.shape[0], -1, np.int64)]))


case(id="left_pad_pairs", symbols=("left_pad",), make=_pad_make, ref=_pad_ref,
     canon=lambda out, _inp: (out[0].astype(np.int64), out[1].astype(np.int64)),
     run=lambda eng, bufs, _p: eng.left_pad_pairs(bufs["ra"], bufs["rb"], PAD_ROWS))

# ---- per pair
TAKE_ROWS, N_IDS = 5000, 10_000


def _ids(r, n_rows, n=N_IDS, none=True):
    idx = r.integers(0, n_rows, n).astype(np.int32)
    if none:
        idx[r.integers(0, n, 20)] = -1     # NEAREST's "none": zero-filled
    return idx


def _take_make(seed):
    r = np.random.default_rng(seed)
    return {"c1": r.integers(-100, 100, TAKE_ROWS).astype(np.int8), "c4": r.integers(0, 2**31 - 1, TAKE_ROWS).astype(np.int32),
            "c8": r.standard_normal(TAKE_ROWS), "c16": (r.standard_normal(TAKE_ROWS) + 1j * r.standard_normal(TAKE_ROWS)),
            "idx": _ids(r, TAKE_ROWS, N_IDS + 1)}


TAKE_COLS = ("c1", "c4", "c8", "c16")


def _take_ref(inp, first):
    idx = inp["idx"][first:]
    return tuple(np.where(idx >= 0, inp[c][np.maximum(idx, 0)], 0).astype(inp[c].dtype) for c in TAKE_COLS)


case(id="take[vector]", symbols=("take",), make=_take_make, ref=lambda inp: _take_ref(inp, 0), canon=_identity,
     run=lambda eng, bufs, _p: eng.take([bufs[c] for c in TAKE_COLS], bufs["idx"]))
case(id="take[scalar]", symbols=("take",), make=_take_make, ref=lambda inp: _take_ref(inp, 1), canon=_identity,
     run=lambda eng, bufs, _p: eng.take([bufs[c] for c in TAKE_COLS], bufs["idx"][1:]))      # a 4-byte-offset view

UTF8_LENGTHS = [0, 31, 32, 33, 300] * 100


def _utf8_make(seed):
    r = np.random.default_rng(seed)
    off, data = utf8_column(r, UTF8_LENGTHS)
    return {"off": off, "data": data, "idx": _ids(r, len(UTF8_LENGTHS))}


def _utf8_ref(inp):
    rows = utf8_rows(inp["off"], inp["data"])
    return tuple(rows[i] if i >= 0 else b"" for i in inp["idx"])


case(id="take_utf8", symbols=("take_utf8_plan", "take_utf8_fill"), make=_utf8_make, ref=_utf8_ref,
     canon=lambda out, _inp: tuple(utf8_rows(out[0], out[1])),
     run=lambda eng, bufs, _p: eng.take_utf8(bufs["off"], bufs["data"], bufs["idx"]))


def _select_make(seed):
    r = np.random.default_rng(seed)
    return {"ia": _ids(r, TAKE_ROWS, none=False), "ib": _ids(r, TAKE_ROWS, none=False),
            "ca": r.integers(-1000, 1000, TAKE_ROWS).astype(np.int32), "ca.valid": (r.random(TAKE_ROWS) >= 0.3).astype(np.uint8),
            "cb": r.normal(0, 700, TAKE_ROWS), "cl": r.integers(-2**40, 2**40, TAKE_ROWS).astype(np.int64)}


def _select_ref(inp):
    ia, ib = inp["ia"], inp["ib"]
    keep = (inp["ca.valid"][ia] != 0) & (inp["ca"][ia] < inp["cb"][ib])      # NULL < x is not true
    return ia[keep], ib[keep]


def _select_preds(bufs):
    return [(("a", bufs["ca"], bufs["ca.valid"]), "<", ("b", bufs["cb"]))]


def _select_raw(eng, bufs, _p):
    """``giql_hip_select_dev``: the engine's ``select`` goes through ``giql_hip_select_expr_dev`` only."""
    import torch
    from giql_amd import _lib

    c_preds, k, _keep, _nodes, _n = eng._c_preds(_select_preds(bufs))
    out_a = torch.empty(N_IDS, dtype=torch.int32, device=eng.device)
    out_b = torch.empty(N_IDS, dtype=torch.int32, device=eng.device)
    kept = ctypes.c_int64(0)
    _lib.check(eng._L.giql_hip_select_dev(eng._h, c_preds, k, bufs["ia"].data_ptr(), TAKE_ROWS, bufs["ib"].data_ptr(),
                                          TAKE_ROWS, N_IDS, out_a.data_ptr(), out_b.data_ptr(), ctypes.byref(kept),
                                          eng._stream()))
    return out_a[: kept.value], out_b[: kept.value]


case(id="select", symbols=("select_expr",), make=_select_make, ref=_select_ref, canon=_identity,
     run=lambda eng, bufs, _p: eng.select(_select_preds(bufs), idx_a=bufs["ia"], idx_b=bufs["ib"], n_rows_a=TAKE_ROWS,
                                          n_rows_b=TAKE_ROWS))
case(id="select[raw]", symbols=("select",), make=_select_make, ref=_select_ref, canon=_identity, run=_select_raw)


def _eval_ref(inp):
    ia, ib = inp["ia"], inp["ib"]
    ok = inp["ca.valid"][ia] != 0
    total = inp["ca"][ia].astype(np.int64) + inp["cl"][ib] * 3
    over = ok & (inp["cb"][ib] > 0)       # the NULL of ca makes the whole condition NULL: the searched CASE takes ELSE
    return ((np.where(ok, total, 0), ok.astype(np.uint8)),
            (np.where(over, inp["ca"][ia].astype(np.int64), -1), None))


def _eval_run(eng, bufs, _p):
    ca = ("a", bufs["ca"], bufs["ca.valid"])
    trees = [("+", ca, ("*", ("b", bufs["cl"]), ("lit", 3))),
             ("if", ("and", ("notnull", ca), (">", ("b", bufs["cb"]), ("lit", 0))), ca, ("lit", -1))]
    return eng.eval_exprs(trees, idx_a=bufs["ia"], idx_b=bufs["ib"], n_rows_a=TAKE_ROWS, n_rows_b=TAKE_ROWS)


case(id="eval_exprs", symbols=("eval_expr",), make=_select_make, ref=_eval_ref, canon=_identity, run=_eval_run)

# ---- aggregates over a join's pairs per left row: ids in, one row per A row out
PAGG_NA, PAGG_NB, PAGG_PAIRS = 40, 600, 5000
PAGG_AGGS = (("SUM", "vf"), ("AVG", "vf"), ("MIN", "vf"), ("MAX", "vf"), ("COUNT", "vf"), ("SUM", "vi"), ("MIN", "vi"),
             ("MAX", "vi"))


def _pagg_make(seed):
    """~5,000 pairs of a 40 x 600 join (every id in range, none -1, some pairs twice), a nullable float64 and an int64
    column of B, a nullable int64 column of A (read by the expression case only)."""
    r = np.random.default_rng(seed)
    return {"ra": r.integers(0, PAGG_NA, PAGG_PAIRS).astype(np.int32), "rb": r.integers(0, PAGG_NB, PAGG_PAIRS).astype(np.int32),
            "vf": (r.normal(0, 1000, PAGG_NB) * r.choice([1e-3, 1.0, 1e3], PAGG_NB)).astype(np.float64),
            "vf.valid": (r.random(PAGG_NB) >= 0.3).astype(np.uint8),
            "vi": r.integers(-1_000_000, 1_000_000, PAGG_NB).astype(np.int64),
            "ca": r.integers(-1000, 1000, PAGG_NA).astype(np.int64), "ca.valid": (r.random(PAGG_NA) >= 0.3).astype(np.uint8)}


def _py_column(inp, name):
    ok = inp[name + ".valid"] if name + ".valid" in inp else np.ones(inp[name].shape[0], np.uint8)
    return [v.item() if k else None for v, k in zip(inp[name], ok)]


def _pagg_leaf(func, want, inputs, flt):
    """One aggregate of the reference as ``(values, non_null)``: NULL reads 0; a float SUM of k values carries
    ``_agg_ref``'s bound k * 2^-52 * sum|x|, a float AVG that over k plus one ulp of the result; the rest is exact."""
    import _pair_agg_ref as R

    nn = np.array([sum(x is not None for x in xs) for xs in inputs], np.int64)
    vals = [0 if w is None else w for w in want]
    if func == "COUNT":
        return np.array(vals, np.int64), nn
    if not (flt or func == "AVG"):
        return np.array(vals, np.int64), nn
    bounds = []
    for w, xs, k in zip(want, inputs, nn.tolist()):
        bound = 0.0
        if w is not None and flt and func in ("SUM", "AVG"):
            bound = k * 2.0 ** -52 * R.abs_sum(xs)
            bound = bound if func == "SUM" else bound / k + math.ulp(w)
        bounds.append(bound)
    return Approx(np.array(vals, np.float64), bounds), nn


def _pagg_ref(inp):
    import _pair_agg_ref as R

    cols = {name: _py_column(inp, name) for name in ("vf", "vi")}
    pairs, results = R.pair_aggregate(inp["ra"], inp["rb"], PAGG_NA, cols, [(f, c) for f, c in PAGG_AGGS])
    mem = R.members(inp["ra"], inp["rb"], PAGG_NA)
    return (np.array(pairs, np.int64),) + tuple(
        _pagg_leaf(f, want, [[cols[c][b] for b in m] for m in mem], c == "vf") for (f, c), want in zip(PAGG_AGGS, results))


def _pagg_canon(out, _inp):
    pairs, results = out
    return (np.asarray(pairs),) + tuple((np.asarray(v), np.asarray(nn)) for v, nn in results)


def _pagg_run(eng, bufs, _p):
    valid = {"vf": bufs["vf.valid"], "vi": None}
    return eng.pair_aggregate(bufs["ra"], bufs["rb"], PAGG_NA, PAGG_NB, [(f, bufs[c], valid[c]) for f, c in PAGG_AGGS])


case(id="pair_aggregate", symbols=("pair_agg",), make=_pagg_make, ref=_pagg_ref, canon=_pagg_canon, run=_pagg_run)

PXAGG_FUNCS = ("SUM", "MAX", "COUNT", "AVG")     # of the tree ``a.ca + b.vi * 3`` (a NULL ``a.ca``: no input); then SUM(b.vf)


def _pxagg_tree(inp):
    return ("+", ("a", inp["ca"], inp["ca.valid"]), ("*", ("b", inp["vi"]), ("lit", 3)))


def _pxagg_ref(inp):
    import _pair_expr_agg_ref as X

    tree = _pxagg_tree({k: np.asarray(v) for k, v in inp.items()})
    plain = ("col", _py_column(inp, "vf"))
    aggs = [(f, tree) for f in PXAGG_FUNCS] + [("SUM", plain)]
    pairs, results, inputs = X.pair_expr_aggregate(inp["ra"], inp["rb"], PAGG_NA, aggs)
    return (np.array(pairs, np.int64),) + tuple(
        _pagg_leaf(f, want, xs, src is plain) for (f, src), want, xs in zip(aggs, results, inputs))


def _pxagg_run(eng, bufs, _p):
    tree = ("expr", _pxagg_tree(bufs))
    return eng.pair_aggregate(bufs["ra"], bufs["rb"], PAGG_NA, PAGG_NB,
                              [(f, tree) for f in PXAGG_FUNCS] + [("SUM", bufs["vf"], bufs["vf.valid"])])


case(id="pair_aggregate[expr]", symbols=("pair_expr_agg",), make=_pagg_make, ref=_pxagg_ref, canon=_pagg_canon, run=_pxagg_run)

RANGE_SETS = [("intersects", [0, 1, 3], [40_000, 90_000, 70_000], [10_000, 60_000, 65_000]),      # (op, codes, hi, lo)
              ("within", [0, 2], [20_000, 0], [21_000, 50_000]),
              ("contains", [1, 4], [30_020, 5_010], [30_030, 5_015])]


def _range_make(seed):
    out = one_table()(seed)
    out["a.start.valid"] = (np.random.default_rng(seed + 9).random(5000) >= 0.1).astype(np.uint8)
    return out


def _range_ref(inp):
    import _range_set_ref as ref

    ones = np.ones(inp["a.chrom"].shape[0], bool)
    return tuple(tuple(np.asarray(x, np.uint8) for x in ref.any_over_bounds(
        op, inp["a.chrom"], inp["a.start"], inp["a.end"], ones, inp["a.start.valid"] != 0, ones, codes, on_start, on_end))
        for op, codes, on_start, on_end in RANGE_SETS)


case(id="range_set_any", symbols=("range_set_any",), make=_range_make, ref=_range_ref, canon=_identity,
     run=lambda eng, bufs, _p: eng.range_set_any(bufs["a.chrom"], bufs["a.start"], bufs["a.end"], RANGE_SETS,
                                                 valid=(None, bufs["a.start.valid"], None)))


MARK_ROWS = 40_000


def _mark_ref(inp):
    flags = np.zeros(MARK_ROWS, np.uint8)
    flags[inp["idx"]] = 1
    return flags


case(id="mark", symbols=("mark",), canon=_identity, ref=_mark_ref,
     make=lambda seed: {"idx": np.random.default_rng(seed).integers(0, MARK_ROWS, N_IDS).astype(np.int32)},
     run=lambda eng, bufs, _p: eng.mark(bufs["idx"], MARK_ROWS))
case(id="pairs_checksum", symbols=("pairs_checksum",), canon=_identity,
     make=lambda seed: {"ra": _ids(np.random.default_rng(seed), 3000, none=False),
                        "rb": _ids(np.random.default_rng(seed + 1), 20_000, none=False)},
     ref=lambda inp: int(ora.c_pairs_checksum(inp["ra"], inp["rb"])),
     run=lambda eng, bufs, _p: eng.pairs_checksum(bufs["ra"], bufs["rb"]))

# ---- the table index
INDEX_SEED = 7300


@functools.lru_cache(maxsize=None)
def index_tables():
    """The tables the index cases hold fixed: the indexed one (and a query for the case that builds the index)."""
    return two_tables("general")(INDEX_SEED)


def _only(prefix):
    def make(seed):
        return {k: v for k, v in two_tables("general")(seed).items() if k.startswith(prefix)}

    return make


def _index_prepare(eng):
    """Built on the default stream before step 1 (the protocol's first synchronisation is behind it)."""
    from test_gpu_parity import dev

    b = dev(hside(index_tables(), "b"))
    index = eng.index_create(b, 4)
    index.prepare_rows()
    index.prepare_nearest()
    return index, b


def _fixed_b():
    return hside(index_tables(), "b")


case(id="inner_join_indexed", symbols=("inner_join_indexed",), make=_only("a."), prepare=_index_prepare, canon=_pairs_canon,
     ref=lambda inp: sort_pairs(*ora.c_inner(hside(inp, "a"), _fixed_b(), "sweep")),
     run=lambda eng, bufs, p: eng.inner_join_indexed(dside(bufs, "a"), p[0]))
case(id="count_overlaps_indexed", symbols=("count_indexed",), make=_only("a."), prepare=_index_prepare, canon=_identity,
     ref=lambda inp: np.asarray(ora.c_count(hside(inp, "a"), _fixed_b(), "sweep")),
     run=lambda eng, bufs, p: eng.count_overlaps_indexed(dside(bufs, "a"), p[0]))
case(id="semi_anti_indexed", symbols=("semi_anti_indexed",), make=_only("a."), prepare=_index_prepare, canon=_identity,
     ref=lambda inp: tuple(np.sort(ora.c_semi_anti(hside(inp, "a"), _fixed_b(), anti)) for anti in (False, True)),
     run=lambda eng, bufs, p: tuple(eng.semi_anti_indexed(dside(bufs, "a"), p[0], anti) for anti in (False, True)))
case(id="nearest_indexed", symbols=("nearest_indexed",), make=_only("a."), prepare=_index_prepare,
     ref=lambda inp: matched(_fixed_b(), *ora.c_nearest_k1(hside(inp, "a"), _fixed_b(), method="sweep")),
     canon=lambda out, _inp: matched(_fixed_b(), out[0], out[1]),
     run=lambda eng, bufs, p: eng.nearest_indexed(dside(bufs, "a"), p[0]))


def _index_create_run(eng, bufs, query):
    index = eng.index_create(dside(bufs, "b"), 4)
    index.prepare_rows()
    index.prepare_nearest()
    counts = eng.count_overlaps_indexed(query, index)
    idx, dist = eng.nearest_indexed(query, index)
    return counts, idx, dist, index      # (the index lives as long as the result: nothing of it is freed under the call)


def _index_create_ref(inp):
    a, b = hside(index_tables(), "a"), hside(inp, "b")
    return (np.asarray(ora.c_count(a, b, "sweep")),) + matched(b, *ora.c_nearest_k1(a, b, method="sweep"))


def _query_prepare(eng):
    from test_gpu_parity import dev

    return dev(hside(index_tables(), "a"))


case(id="index_create", symbols=("index_create", "index_prepare_rows", "index_prepare_nearest", "count_indexed",
                                 "nearest_indexed"),
     make=_only("b."), prepare=_query_prepare, ref=_index_create_ref, run=_index_create_run,
     canon=lambda out, inp: (out[0],) + matched(hside(inp, "b"), out[1], out[2]))

# ---- a genome wider than the 32-bit axis: HipEngine._wide loops several calls on the stream
WIDE_ENC = ("0based", "half_open")


def _wide_make(seed):
    from test_axis_edges import make_side

    out = {}
    _put(out, "a", make_side("tight_over", WIDE_ENC, 300, seed))
    _put(out, "b", make_side("tight_over", WIDE_ENC, 400, seed + 1))
    out["vi"] = np.random.default_rng(seed + 2).integers(-1_000_000, 1_000_000, 300).astype(np.int64)
    out["vi.valid"] = (np.random.default_rng(seed + 3).random(300) >= 0.3).astype(np.uint8)
    return out


case(id="inner_join[wide]", symbols=("chrom_spans", "inner_plan", "inner_fill"), make=_wide_make, ref=inner_pairs,
     canon=_pairs_canon, run=lambda eng, bufs, _p: eng.inner_join(dside(bufs, "a"), dside(bufs, "b"), 2))
case(id="merge_agg[wide]", symbols=("chrom_spans", "merge_agg"), make=_wide_make, canon=_agg_canon,
     ref=lambda inp: _agg_ref({k: v for k, v in inp.items() if not k.startswith("vf")}, 0),
     run=lambda eng, bufs, _p: eng.merge_agg(dside(bufs, "a"), 2, 0, [(f, bufs["vi"], bufs["vi.valid"]) for f in AGG_FUNCS]))
case(id="coverage[wide]", symbols=("chrom_spans", "coverage"), make=_wide_make, ref=_coverage_ref, canon=_coverage_canon,
     run=lambda eng, bufs, _p: eng.coverage(dside(bufs, "a"), 2))      # (one call per chromosome group, then wide.merge)


# ---------------------------------------------------------------------------------------------- the ABI's stream entry points
#: the two bandwidth probes: they return one GB/s figure, which has no checkable value
NO_CHECKABLE_OUTPUT = ("copy_probe", "stream_probe")


def abi_symbols():
    """Every symbol ``giql_amd/_lib.py`` binds: its module-level lists named ``SYMBOLS`` or ``..._SYMBOLS``, in the
    order the module defines them -- found by name, so that the list of the next extension header is one of them
    without an edit here.  The completeness gates of tests/test_streams_gpu.py and tests/test_plan_lifetime_gpu.py
    both run over this."""
    from giql_amd import _lib

    lists = [v for k, v in vars(_lib).items() if (k == "SYMBOLS" or k.endswith("_SYMBOLS")) and isinstance(v, (list, tuple))]
    assert lists and all(isinstance(s, str) and s.startswith("giql_hip_") for symbols in lists for s in symbols)
    return [s for symbols in lists for s in symbols]


def stream_entry_points():
    """Every function a header ``include/giql_hip*.h`` declares with a ``void* stream`` parameter, under its full
    name (``_lib.py``'s prototypes are lists of ctypes types: the headers name the parameter)."""
    out = []
    for path in sorted(glob.glob(os.path.join(os.path.dirname(HERE), "include", "giql_hip*.h"))):
        with open(path) as f:
            text = re.sub(r"/\*.*?\*/", "", re.sub(r"//[^\n]*", "", f.read()), flags=re.S)
        for m in re.finditer(r"\b(giql_hip_\w+)\s*\(([^;{]*)\)\s*;", text):
            if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2)):
                out.append(m.group(1))
    return out


def short(symbol):
    name = symbol[len("giql_hip_"):]
    return name[:-4] if name.endswith("_dev") else name
