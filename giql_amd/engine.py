"""Device-resident engine: torch tensors in, torch tensors out, arithmetic in HIP.

torch is used only as plumbing (device memory, the current stream); every result
comes from ``libgiql_hip.so`` through the C ABI of ``include/giql_hip.h``.

Reference interface mirrored (path:line under /root/reference/):
the per-chromosome INNER / SEMI / ANTI plans of
``src/giql/expanders/intersects_duckdb.py:1254-1330``, count_overlaps
(``:806-854``) and NEAREST k=1 (``src/giql/expanders/nearest.py:336-397``), with
each table's coordinate encoding applied as in ``src/giql/canonical.py:16-52``.
"""

from __future__ import annotations

import ctypes
from dataclasses import dataclass

from . import _lib, wide

#: (coordinate_system, interval_type) -> (start_off, end_off)
#: src/giql/canonical.py:16-52
ENCODING_OFFSETS = {
    ("0based", "half_open"): (0, 0),
    ("0based", "closed"): (0, +1),
    ("1based", "half_open"): (-1, -1),
    ("1based", "closed"): (-1, 0),
}


def _torch():
    import torch

    return torch


def expr_can_float(tree) -> bool:
    """The static type of an expression tree as :meth:`HipEngine.eval_exprs` takes it: can its value be a float?
    The rule ``giql_hip_eval_expr_dev`` checks on the host (include/giql_hip.h): a float32 / float64 column or a
    float literal is, the result of ``/`` is, arithmetic / ``neg`` / ``abs`` / ``least`` / ``greatest`` are when an
    argument is, ``if`` when its ``then`` or ``else`` is; comparisons, IS [NOT] NULL, AND / OR / NOT and ``null``
    are integers.  A float-typed expression needs a float64 output, every other one is int64."""
    kind = tree[0]
    if kind == "expr":
        return expr_can_float(tree[1])
    if kind == "lit":
        return isinstance(tree[1], float)
    if kind in ("a", "b"):
        return bool(tree[1].dtype.is_floating_point)
    if kind == "/":
        return True
    if kind == "if":
        return expr_can_float(tree[2]) or expr_can_float(tree[3])
    if kind in ("+", "-", "*", "neg", "abs", "least", "greatest"):
        return any(expr_can_float(c) for c in tree[1:])
    return False


def _c_max_distance(max_distance) -> int:
    """``max_distance`` as the C ABI takes it: -1 = no limit."""
    return -1 if max_distance is None else int(max_distance)


@dataclass
class DeviceSide:
    """One join side resident in HBM: int32 chrom ids / start / end tensors."""

    chrom: "object"
    start: "object"
    end: "object"
    start_off: int = 0
    end_off: int = 0

    def __post_init__(self) -> None:
        torch = _torch()
        for name in ("chrom", "start", "end"):
            t = getattr(self, name)
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 1:
                raise ValueError(f"{name} must be a 1-D torch.int32 tensor")
            if not t.is_cuda:
                raise ValueError(f"{name} must live on the GPU (cuda/hip device)")
            if not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
        if not (self.chrom.shape == self.start.shape == self.end.shape):
            raise ValueError("chrom/start/end lengths differ")

    @property
    def n(self) -> int:
        return int(self.chrom.shape[0])

    @property
    def device(self):
        return self.chrom.device

    @classmethod
    def from_numpy(cls, chrom, start, end, encoding=("0based", "half_open"), device="cuda:0"):
        import numpy as np

        torch = _torch()
        so, eo = ENCODING_OFFSETS[tuple(encoding)]

        def up(x):
            x = np.ascontiguousarray(x, dtype=np.int32)
            if x.flags.writeable:
                return torch.from_numpy(x).to(device)
            # read-only memory (cached chromosome ids, read-only Arrow buffers): torch warns about aliasing it; the
            # host tensor here is only ever READ, by the upload on the next line, and dropped
            import warnings

            with warnings.catch_warnings():
                warnings.simplefilter("ignore", UserWarning)
                return torch.from_numpy(x).to(device)

        return cls(up(chrom), up(start), up(end), so, eo)

    def c_struct(self) -> _lib.CSide:
        n = self.n
        return _lib.CSide(
            self.chrom.data_ptr() if n else None,
            self.start.data_ptr() if n else None,
            self.end.data_ptr() if n else None,
            n, self.start_off, self.end_off)


class DeviceIndex:
    """A table index in HBM (``giql_hip_index``): what the reference's users get from ``CREATE INDEX ... (chrom,
    start, "end")`` (``docs/transpilation/performance.rst:111-130``).  Built by :meth:`HipEngine.index_create`,
    used by :meth:`HipEngine.inner_join_indexed`, :meth:`HipEngine.count_overlaps_indexed`,
    :meth:`HipEngine.semi_anti_indexed` and :meth:`HipEngine.nearest_indexed`; released by :meth:`close` / garbage
    collection."""

    def __init__(self, engine: "HipEngine", handle, n_chrom: int):
        self.engine, self._h, self.n_chrom, self.last_pairs = engine, handle, n_chrom, 0
        self._refresh_info()

    def _info(self):
        n, b, g, sp = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int64(0)
        _lib.check(self.engine._L.giql_hip_index_info(self._h, ctypes.byref(n), ctypes.byref(b), ctypes.byref(g), ctypes.byref(sp)))
        return int(n.value), int(b.value), bool(g.value), int(sp.value)

    def _refresh_info(self) -> None:
        self.n, _, self.general, self.span = self._info()   # fixed at creation

    @property
    def nbytes(self) -> int:
        """HBM bytes of the arrays the index owns now (``giql_hip_index_info``): grows when a preparation adds its
        arrays, whoever ran it."""
        return self._info()[1]

    def prepare_rows(self) -> None:
        """Build what the per-row operators read of the index (``giql_hip_index_prepare_rows_dev``: a directory of
        bucket boundaries; for a table of variable length its sorted end keys too, 4 B per row).  Once per index
        -- a second call does nothing -- and done by the first ``count_overlaps_indexed`` / ``semi_anti_indexed``
        call otherwise."""
        eng = self.engine
        _lib.check(eng._L.giql_hip_index_prepare_rows_dev(eng._h, self._h, eng._stream()))

    def prepare_nearest(self) -> None:
        """Build what :meth:`HipEngine.nearest_indexed` reads of the index (``giql_hip_index_prepare_nearest_dev``:
        the directory of bucket boundaries it shares with the row operators, a rank per chromosome; for a table of
        variable length the row ids and the prefix max of the ends in (start, end) order too, 8 B per row).  Once
        per index -- a second call does nothing -- and done by the first ``nearest_indexed`` call otherwise.
        ``GIQL_ERR_STATE`` (now and on every later NEAREST call) when a table of variable
        length holds a long run of rows on one start: the ordinary operator answers such a table."""
        eng = self.engine
        _lib.check(eng._L.giql_hip_index_prepare_nearest_dev(eng._h, self._h, eng._stream()))

    def close(self) -> None:
        if getattr(self, "_h", None):
            self.engine._L.giql_hip_index_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass


class InvertedRows(ValueError):
    """A side of a within-distance join holds a row with ``start > end``.  ``sides``: which -- ``"a"``, ``"b"`` or
    both -- as the library reports them in its stats (``n_irregular_a`` / ``n_irregular_b`` = -1), not read off the
    wording of its message."""

    def __init__(self, sides: tuple, message: str):
        super().__init__(message)
        self.sides = tuple(sides)


#: left rows one block of the LEFT OUTER pad's count / fill kernels covers (csrc/outer_kernels.hip.h, LP_BLOCK_ROWS)
LEFT_PAD_BLOCK_ROWS = 32768


class HipEngine:
    """One context (device arena + bookkeeping) on one GPU.  Not thread-safe."""

    def __init__(self, device: int = 0, profiling: bool = False):
        self._L = _lib.load()
        torch = _torch()
        if not torch.cuda.is_available():
            raise _lib.GiqlHipUnavailable("no HIP device visible to torch; there is no CPU fallback")
        self.device_index = int(device)
        self.device = torch.device("cuda", self.device_index)
        h = ctypes.c_void_p()
        _lib.check(self._L.giql_hip_create(self.device_index, ctypes.byref(h)))
        self._h = h
        self.set_profiling(profiling)

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.giql_hip_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------- utilities
    def _stream(self):
        torch = _torch()
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def set_profiling(self, enabled) -> None:
        """``False`` / ``True`` (hipEvent pairs around every phase) / ``2`` (only around the sort passes) /
        a phase name of ``_lib.PHASES`` (only around that phase)."""
        if isinstance(enabled, str):
            enabled = 16 + _lib.PHASES.index(enabled)
        _lib.check(self._L.giql_hip_set_profiling(self._h, int(enabled)))

    def reserve(self, nbytes: int) -> None:
        _lib.check(self._L.giql_hip_reserve(self._h, int(nbytes)))

    def stats(self) -> dict:
        st = _lib.CStats()
        _lib.check(self._L.giql_hip_get_stats(self._h, ctypes.byref(st)))
        out = {k: int(getattr(st, k)) for k in
               ("n_a", "n_b", "n_out", "n_irregular_a", "n_irregular_b", "workspace_bytes", "span",
                "profiled")}
        out["join_form"] = {0: "general", 1: "uniform_b", 2: "uniform_a"}.get(int(st.reserved) & 0x0F, "?")
        out["span_hist"] = bool(int(st.reserved) & 0x10)  # fixed-length side sorted from its raw columns
        out["coarse_b"] = out["span_hist"]  # (SEMI / ANTI / COUNT: the same bit says B was sorted without its lowest digit)
        out["sort_local"] = bool(int(st.reserved) & 0x20)   # a side was sorted in three stages (bucket_sort.hip.h)
        out["sort_resorted"] = bool(int(st.reserved) & 0x40)  # the context fell back to the four-pass sort
        out["swapped"] = bool(int(st.reserved) & 0x80)  # the INNER plan ran with the sides exchanged (larger side as B)
        out["sort_tile_order"] = (int(st.reserved) >> 8) & 0x7F
        out["count_fused"] = bool(int(st.reserved) & 0x8000)  # the bucket sort answered the range bounds (no count kernel)
        out["sort_order_fallbacks"] = (int(st.reserved) >> 16) & 0x7FF
        out["bucket_bits"] = 16 - ((int(st.reserved) >> 27) & 3)  # key bits of a bucket of the last three-stage sort
        out["bucket_join"] = bool((int(st.reserved) >> 29) & 1)  # the bucket stage wrote the pairs itself (one-call form)
        out["fused_fill"] = bool((int(st.reserved) >> 30) & 1)  # the last plan launched its own fill
        out["presorted"] = bool(int(st.reserved) & 0x80000000)  # a side arrived sorted and skipped its sort
        out["total_ms"] = float(st.total_ms)
        out["phase_ms"] = {name: float(st.phase_ms[i]) for i, name in enumerate(_lib.PHASES)}
        out["phase_launches"] = {name: int(st.phase_launches[i]) for i, name in enumerate(_lib.PHASES)}
        out["phase_bytes"] = {name: int(st.phase_bytes[i]) for i, name in enumerate(_lib.PHASES)}
        return out

    def _dev_ptr(self, t, what: str, dtype=None):
        """Device pointer of a tensor argument, or None for an empty one.  Anything that does not live
        on THIS engine's device is refused here: a host pointer handed to a kernel is a GPU memory
        fault, not an exception."""
        if t is None or int(t.numel()) == 0:
            return None
        if not t.is_cuda or t.device != self.device:
            raise ValueError(f"{what} lives on {t.device}, the engine on {self.device}")
        if not t.is_contiguous():
            raise ValueError(f"{what} must be contiguous")
        if dtype is not None and t.dtype != dtype:
            raise ValueError(f"{what} must be {dtype}, got {t.dtype}")
        return t.data_ptr()

    def _check_sides(self, a: DeviceSide, b: DeviceSide) -> None:
        for s in (a, b):
            if s.n and s.device != self.device:
                raise ValueError(f"side lives on {s.device}, engine on {self.device}")

    # ------------------------------------------------------------------ INNER
    def inner_plan(self, a: DeviceSide, b: DeviceSide, n_chrom: int) -> int:
        self._check_sides(a, b)
        n = ctypes.c_int64(0)
        ca, cb = a.c_struct(), b.c_struct()
        _lib.check(self._L.giql_hip_inner_plan_dev(self._h, ca, cb, int(n_chrom), self._stream(),
                                                   ctypes.byref(n)))
        self._keepalive = (a, b)
        return int(n.value)

    def inner_fill(self, row_a, row_b) -> None:
        torch = _torch()
        cap = min(int(row_a.shape[0]), int(row_b.shape[0]))
        _lib.check(self._L.giql_hip_inner_fill_dev(
            self._h, self._dev_ptr(row_a, "row_a", torch.int32), self._dev_ptr(row_b, "row_b", torch.int32), cap,
            self._stream()))

    def inner_join_into(self, a: DeviceSide, b: DeviceSide, n_chrom: int, row_a, row_b) -> int:
        """Plan + fill into caller-owned int32 tensors in ONE C-ABI call (no stream sync between
        the two when the context's guesses hold); returns the pair count.  Raises
        :class:`GiqlHipError` with ``GIQL_ERR_CAPACITY`` when the buffers are too small (the
        plan stays valid for :meth:`inner_fill`)."""
        self._check_sides(a, b)
        cap = min(int(row_a.shape[0]), int(row_b.shape[0]))
        n = ctypes.c_int64(0)
        self.last_pairs = None
        torch = _torch()
        rc = self._L.giql_hip_inner_join_dev(
            self._h, a.c_struct(), b.c_struct(), int(n_chrom), self._dev_ptr(row_a, "row_a", torch.int32),
            self._dev_ptr(row_b, "row_b", torch.int32), cap, self._stream(), ctypes.byref(n))
        self.last_pairs = int(n.value)
        _lib.check(rc)
        return int(n.value)

    def inner_join(self, a: DeviceSide, b: DeviceSide, n_chrom: int, out=None):
        """All ``(row_a, row_b)`` with ``a INTERSECTS b``; two int32 device tensors."""
        row_a, row_b, n = self._join_into_buffers(a, b, n_chrom, out=out)
        return row_a[:n], row_b[:n]

    def _join_into_buffers(self, a: DeviceSide, b: DeviceSide, n_chrom: int, out=None, extra_room: int = 0):
        """The INNER join's pairs at the front of two int32 device buffers: ``(row_a, row_b, n_pairs)``.  The buffers
        hold at least ``n_pairs + extra_room`` entries (what a caller appends behind the pairs: :meth:`left_join`),
        and the join itself is never offered the extra room -- except on a genome wider than the 32-bit axis, when
        the pairs of the chromosome groups come back in tensors of exactly their length (:meth:`_wide`).  A group's
        join is planned and filled into exactly sized buffers and leaves ``_pairs_guess`` / ``_pairs_guess_rows``
        alone: a sub-join must not overwrite the guess of the whole."""
        torch = _torch()

        def once(sa, sb, rows):
            if rows is None:
                return self._join_once(sa, sb, n_chrom, out, int(extra_room))
            n = self.inner_plan(sa, sb, n_chrom)
            pairs = [torch.empty(n, dtype=torch.int32, device=self.device) for _ in range(2)]
            self.inner_fill(*pairs)
            return pairs

        def combine(parts):
            ra, rb = wide.pairs(parts, self.device)
            return ra, rb, int(ra.shape[0])

        return self._wide(once, combine, a, b, n_chrom)

    def _join_once(self, a: DeviceSide, b: DeviceSide, n_chrom: int, out, extra: int):
        torch = _torch()
        # A context that has joined before gets ONE call (giql_hip_inner_join_dev): buffers sized from its previous
        # result -- for large tables the pairs are then written by the sort's last stage itself, with no count /
        # scan / fill kernels and no read-back in between.  A result that does not fit comes back as
        # GIQL_ERR_CAPACITY with the exact count and a plan behind it: the ordinary fill follows.
        # The guess belongs to the INPUTS it was made on: for tables of another size it is scaled by the product of
        # the row counts (the same density assumed) and never exceeds n_a * n_b or a third of the free HBM -- a
        # guess left by a 404M-pair join must not size the buffers of a 1,000-row sub-join.
        guess = getattr(self, "_pairs_guess", 0)
        g_na, g_nb = getattr(self, "_pairs_guess_rows", (a.n, b.n))
        if guess > 0 and a.n and b.n and (g_na, g_nb) != (a.n, b.n):
            guess = int(guess * (a.n / max(g_na, 1)) * (b.n / max(g_nb, 1))) + 1
        guess = min(guess, a.n * b.n)
        row_a = row_b = None
        cap = 0
        if out is None and guess > 0 and a.n and b.n:
            cap = min(int(guess * 1.05) + 4096, a.n * b.n)
            try:
                free = int(torch.cuda.mem_get_info(self.device)[0])
                cap = min(cap, max(free // 24 - extra, 4096))     # two int32 arrays within a third of what is free
            except Exception:  # pragma: no cover
                pass
            try:   # (a guess left over from a much larger join must not be what runs the device out of memory)
                row_a = torch.empty(cap + extra, dtype=torch.int32, device=self.device)
                row_b = torch.empty(cap + extra, dtype=torch.int32, device=self.device)
            except RuntimeError:
                row_a = row_b = None
                self._pairs_guess = 0
        if row_a is not None and row_b is not None:
            try:
                # (the join sees `cap` entries only: pairs past the guess must not spend the caller's extra room)
                n = self.inner_join_into(a, b, n_chrom, row_a[:cap], row_b[:cap])
                self._pairs_guess, self._pairs_guess_rows = n, (a.n, b.n)
                return row_a, row_b, n
            except _lib.GiqlHipError as exc:
                if exc.code != _lib.GIQL_ERR_CAPACITY:
                    raise
                n = int(self.last_pairs)
                del row_a, row_b
                row_a = torch.empty(n + extra, dtype=torch.int32, device=self.device)
                row_b = torch.empty(n + extra, dtype=torch.int32, device=self.device)
                self.inner_fill(row_a, row_b)
                self._pairs_guess, self._pairs_guess_rows = n, (a.n, b.n)
                return row_a, row_b, n
        n = self.inner_plan(a, b, n_chrom)
        self._pairs_guess, self._pairs_guess_rows = n, (a.n, b.n)
        if out is not None and min(int(out[0].shape[0]), int(out[1].shape[0])) >= n + extra:
            row_a, row_b = out[0], out[1]
        else:
            row_a = torch.empty(n + extra, dtype=torch.int32, device=self.device)
            row_b = torch.empty(n + extra, dtype=torch.int32, device=self.device)
        self.inner_fill(row_a[:n], row_b[:n])
        return row_a, row_b, n

    # ------------------------------------------------------------- table index
    def index_create(self, side: DeviceSide, n_chrom: int) -> "DeviceIndex":
        """Build a :class:`DeviceIndex` over a table (``giql_hip_index_create_dev``): its rows keyed on the linear
        axis, grouped by 65,536-key bucket and sorted, kept in HBM (8 B per row; 12 for variable lengths).  Raises
        ``GiqlHipError`` with ``GIQL_ERR_STATE`` when the table does not take the indexed form."""
        h = ctypes.c_void_p()
        cs = side.c_struct()
        _lib.check(self._L.giql_hip_index_create_dev(self._h, ctypes.byref(cs), int(n_chrom), self._stream(),
                                                     ctypes.byref(h)))
        return DeviceIndex(self, h, int(n_chrom))

    def inner_join_indexed(self, a: DeviceSide, index: "DeviceIndex", cap: int | None = None):
        """``(row_a, row_of_indexed_table)`` int32 device tensors of ``a INTERSECTS indexed table``
        (``giql_hip_inner_join_indexed_dev``).  ``a.chrom`` speaks the indexed table's dictionary.  The buffers
        are sized from the index's previous result (``cap`` overrides); a short buffer costs one more call."""
        torch = _torch()
        self._check_indexed(a, index)
        cap = int(cap) if cap is not None else (int(index.last_pairs * 1.05) + 4096 if index.last_pairs else max(a.n, 1 << 20))
        for _attempt in range(3):
            row_a = torch.empty(cap, dtype=torch.int32, device=self.device)
            row_b = torch.empty(cap, dtype=torch.int32, device=self.device)
            try:
                n = self.inner_join_indexed_into(a, index, row_a, row_b)
            except _lib.GiqlHipError as exc:
                if exc.code != _lib.GIQL_ERR_CAPACITY:
                    raise
                del row_a, row_b
                cap = int(self.last_pairs) + 4096
                continue
            return row_a[:n], row_b[:n]
        raise _lib.GiqlHipError(_lib.GIQL_ERR_CAPACITY, "the pair count kept changing between calls")

    def inner_join_indexed_into(self, a: DeviceSide, index: "DeviceIndex", row_a, row_b) -> int:
        """The same into caller-owned int32 tensors; returns the pair count (``GIQL_ERR_CAPACITY`` with
        ``self.last_pairs`` set when they are too small)."""
        torch = _torch()
        cap = min(int(row_a.shape[0]), int(row_b.shape[0]))
        n = ctypes.c_int64(0)
        ca = a.c_struct()
        rc = self._L.giql_hip_inner_join_indexed_dev(
            self._h, index._h, ctypes.byref(ca), self._dev_ptr(row_a, "row_a", torch.int32),
            self._dev_ptr(row_b, "row_b", torch.int32), cap, self._stream(), ctypes.byref(n))
        self.last_pairs = int(n.value)
        _lib.check(rc)
        index.last_pairs = int(n.value)
        return int(n.value)

    def _check_indexed(self, a: DeviceSide, index: "DeviceIndex") -> None:
        if index.engine is not self:
            raise ValueError("the index was built on another engine")
        if a.n and a.device != self.device:
            raise ValueError(f"side lives on {a.device}, engine on {self.device}")

    def count_overlaps_indexed(self, a: DeviceSide, index: "DeviceIndex"):
        """int64 device tensor: the number of overlapping rows of the indexed table per row of ``a``, in ``a``'s
        order (``giql_hip_count_indexed_dev``: what :meth:`count_overlaps` returns, without sorting either side).
        ``a.chrom`` speaks the indexed table's dictionary.  ``GIQL_ERR_STATE`` when ``a`` holds irregular rows."""
        torch = _torch()
        self._check_indexed(a, index)
        counts = torch.zeros(a.n, dtype=torch.int64, device=self.device)
        ca = a.c_struct()
        rc = self._L.giql_hip_count_indexed_dev(self._h, index._h, ctypes.byref(ca),
                                                counts.data_ptr() if a.n else None, self._stream())
        _lib.check(rc)
        return counts

    def semi_anti_indexed(self, a: DeviceSide, index: "DeviceIndex", anti: bool):
        """Ascending int32 row ids of ``a`` with (SEMI) / without (ANTI) an overlapping row of the indexed table
        (``giql_hip_semi_anti_indexed_dev``: what :meth:`semi_anti` returns).  ``GIQL_ERR_STATE`` when ``a`` holds
        irregular rows."""
        torch = _torch()
        self._check_indexed(a, index)
        rows = torch.empty(a.n, dtype=torch.int32, device=self.device)
        n = ctypes.c_int64(0)
        ca = a.c_struct()
        rc = self._L.giql_hip_semi_anti_indexed_dev(self._h, index._h, ctypes.byref(ca), int(bool(anti)),
                                                    rows.data_ptr() if a.n else None, ctypes.byref(n), self._stream())
        _lib.check(rc)
        return rows[: int(n.value)]

    def nearest_indexed(self, a: DeviceSide, index: "DeviceIndex", signed: bool = False, max_distance=None):
        """NEAREST k=1 of ``a`` over the indexed table: ``(idx_b int32, distance int64)`` per row of ``a``, in
        ``a``'s order; idx_b = -1 = none (``giql_hip_nearest_indexed_dev``: what :meth:`nearest` returns, without
        sorting either side).  ``a.chrom`` speaks the indexed table's dictionary.  ``GIQL_ERR_INVALID`` for a row
        with end < start; ``GIQL_ERR_STATE`` when the index does not take the NEAREST form
        (:meth:`DeviceIndex.prepare_nearest`)."""
        torch = _torch()
        self._check_indexed(a, index)
        # (the library writes every slot; one spare element keeps the pointers non-NULL for an empty query)
        idx = torch.empty(max(a.n, 1), dtype=torch.int32, device=self.device)
        dist = torch.empty(max(a.n, 1), dtype=torch.int64, device=self.device)
        md = _c_max_distance(max_distance)
        ca = a.c_struct()
        _lib.check(self._L.giql_hip_nearest_indexed_dev(self._h, index._h, ctypes.byref(ca), int(bool(signed)), md,
                                                        idx.data_ptr(), dist.data_ptr(), self._stream()))
        return idx[: a.n], dist[: a.n]

    # ------------------------------------------------ genomes longer than 2^32
    def chrom_spans(self, a: DeviceSide, b: DeviceSide, n_chrom: int):
        """Per-chromosome coordinate span (host list of ints)."""
        import numpy as np

        self._check_sides(a, b)
        spans = np.zeros(int(n_chrom), np.int64)
        _lib.check(self._L.giql_hip_chrom_spans_dev(
            self._h, a.c_struct(), b.c_struct(), int(n_chrom), spans.ctypes.data, self._stream()))
        return spans.tolist()

    def _groups(self, a: DeviceSide, b: DeviceSide, n_chrom: int, pad: int = 0):
        """Yield ``(sub_a, rows_a, sub_b, rows_b)`` per 32-bit chromosome group (``pad``: positions an operator
        adds to every present chromosome's span -- the within-distance join: 2).

        The kernels place all chromosomes on one u32 axis; a genome whose spans sum
        past 2^32 is joined group by group (chromosomes are independent units).
        Row selection / id mapping here is data plumbing (torch indexing)."""
        torch = _torch()
        from .shard import span_groups

        groups = span_groups([s + pad if s else 0 for s in self.chrom_spans(a, b, n_chrom)])
        for g in groups:
            lut = torch.zeros(int(n_chrom), dtype=torch.bool, device=self.device)
            lut[torch.tensor(g, dtype=torch.long, device=self.device)] = True
            ra = torch.nonzero(lut[a.chrom.long()], as_tuple=False).flatten()
            rb = torch.nonzero(lut[b.chrom.long()], as_tuple=False).flatten()
            sa = DeviceSide(a.chrom[ra].contiguous(), a.start[ra].contiguous(), a.end[ra].contiguous(),
                            a.start_off, a.end_off)
            sb = DeviceSide(b.chrom[rb].contiguous(), b.start[rb].contiguous(), b.end[rb].contiguous(),
                            b.start_off, b.end_off)
            yield sa, ra, sb, rb

    def _empty_side(self) -> DeviceSide:
        torch = _torch()
        z = torch.empty(0, dtype=torch.int32, device=self.device)
        return DeviceSide(z, z.clone(), z.clone(), 0, 0)

    def _wide(self, once, combine, a: DeviceSide, b, n_chrom: int, pad: int = 0):
        """Every operator's answer to a genome wider than the 32-bit axis.  ``once(a, b, None)`` on the whole sides
        is the result; when the library refuses them with ``GIQL_ERR_SPAN``, ``once(sub_a, sub_b, rows_a)`` runs per
        group of :meth:`_groups`, in its order, and ``combine`` (a function of :mod:`giql_amd.wide`) turns the list
        of ``(rows_a, rows_b, result)`` into the result for the whole sides.  ``b=None`` (a one-table operator,
        DISJOIN's self mode): an empty side stands in for the grouping and ``once`` gets ``None`` every time.  Any
        other error is the caller's."""
        try:
            return once(a, b, None)
        except _lib.GiqlHipError as exc:
            if exc.code != _lib.GIQL_ERR_SPAN:
                raise
        groups = self._groups(a, b if b is not None else self._empty_side(), n_chrom, pad)
        return combine([(ra, rb, once(sa, sb if b is not None else None, ra)) for sa, ra, sb, rb in groups])

    # -------------------------------------------------------------- SEMI/ANTI
    def semi_anti(self, a: DeviceSide, b: DeviceSide, n_chrom: int, anti: bool):
        """Ascending A row ids with (SEMI) / without (ANTI) an overlapping B row."""
        self._check_sides(a, b)
        return self._wide(lambda sa, sb, _rows: self._semi_anti_once(sa, sb, n_chrom, anti),
                          lambda parts: wide.row_ids(parts, self.device), a, b, n_chrom)

    def _semi_anti_once(self, a: DeviceSide, b: DeviceSide, n_chrom: int, anti: bool):
        torch = _torch()
        rows = torch.empty(a.n, dtype=torch.int32, device=self.device)
        n = ctypes.c_int64(0)
        _lib.check(self._L.giql_hip_semi_anti_dev(
            self._h, a.c_struct(), b.c_struct(), int(n_chrom), int(bool(anti)),
            rows.data_ptr() if a.n else None, ctypes.byref(n), self._stream()))
        return rows[: int(n.value)]

    def semi_join(self, a, b, n_chrom):
        return self.semi_anti(a, b, n_chrom, False)

    def anti_join(self, a, b, n_chrom):
        return self.semi_anti(a, b, n_chrom, True)

    # ------------------------------------------------------------------ COUNT
    def count_overlaps(self, a: DeviceSide, b: DeviceSide, n_chrom: int):
        """int64 tensor: number of overlapping B rows per A row (original order)."""
        self._check_sides(a, b)
        return self._wide(lambda sa, sb, _rows: self._count_once(sa, sb, n_chrom),
                          lambda parts: wide.per_row(parts, a.n, self.device), a, b, n_chrom)

    def _count_once(self, a: DeviceSide, b: DeviceSide, n_chrom: int):
        torch = _torch()
        counts = torch.zeros(a.n, dtype=torch.int64, device=self.device)
        _lib.check(self._L.giql_hip_count_dev(
            self._h, a.c_struct(), b.c_struct(), int(n_chrom),
            counts.data_ptr() if a.n else None, self._stream()))
        return counts

    # ---------------------------------------------------------------- NEAREST
    def nearest(self, a: DeviceSide, b: DeviceSide, n_chrom: int, signed: bool = False,
                max_distance=None):
        """NEAREST k=1: ``(idx_b int32, distance int64)`` per A row; idx_b=-1 = none."""
        self._check_sides(a, b)
        return self._wide(lambda sa, sb, _rows: self._nearest_once(sa, sb, n_chrom, signed, max_distance),
                          lambda parts: wide.nearest(parts, (a.n,), self.device), a, b, n_chrom)

    def _nearest_once(self, a: DeviceSide, b: DeviceSide, n_chrom: int, signed: bool = False,
                      max_distance=None):
        torch = _torch()
        # (no pre-fill: the library writes every slot -- k_nearest_unpack, or its own memsets for an empty B)
        idx = torch.empty((a.n,), dtype=torch.int32, device=self.device)
        dist = torch.empty(a.n, dtype=torch.int64, device=self.device)
        md = _c_max_distance(max_distance)
        _lib.check(self._L.giql_hip_nearest_dev(
            self._h, a.c_struct(), b.c_struct(), int(n_chrom), int(bool(signed)), md,
            idx.data_ptr() if a.n else None, dist.data_ptr() if a.n else None, self._stream()))
        return idx, dist

    def nearest32(self, a: DeviceSide, b: DeviceSide, n_chrom: int, signed: bool = False, max_distance=None):
        """NEAREST k=1 with the 8-byte-per-row output: an ``[n_a, 2]`` int32 tensor of ``{idx_b, distance}``
        records (``giql_hip_nearest32_dev``; idx_b = -1: none).  Raises ``GiqlHipError`` (GIQL_ERR_INVALID) when a
        distance does not fit int32 -- :meth:`nearest` is the entry for such data; a genome wider than 32 bits
        (GIQL_ERR_SPAN) also belongs there."""
        torch = _torch()
        self._check_sides(a, b)
        out = torch.empty((a.n, 2), dtype=torch.int32, device=self.device)
        md = _c_max_distance(max_distance)
        _lib.check(self._L.giql_hip_nearest32_dev(
            self._h, a.c_struct(), b.c_struct(), int(n_chrom), int(bool(signed)), md,
            out.data_ptr() if a.n else None, self._stream()))
        return out

    def nearest_k(self, a: DeviceSide, b: DeviceSide, n_chrom: int, k: int, signed: bool = False, max_distance=None):
        """NEAREST k >= 1: ``(idx_b [n_a, k] int32, distance [n_a, k] int64)`` per A row in the reference's
        order ABS(distance), start, end; unused slots idx_b = -1 (``giql_hip_nearest_k_dev``)."""
        self._check_sides(a, b)
        k = int(k)
        return self._wide(lambda sa, sb, _rows: self._nearest_k_once(sa, sb, n_chrom, k, signed, max_distance),
                          lambda parts: wide.nearest(parts, (a.n, k), self.device), a, b, n_chrom)

    def _nearest_k_once(self, a: DeviceSide, b: DeviceSide, n_chrom: int, k: int, signed: bool = False,
                        max_distance=None):
        torch = _torch()
        # (no pre-fill: the library writes every slot, unused ones as idx -1 / distance 0)
        idx = torch.empty((a.n, k), dtype=torch.int32, device=self.device)
        dist = torch.empty((a.n, k), dtype=torch.int64, device=self.device)
        md = _c_max_distance(max_distance)
        _lib.check(self._L.giql_hip_nearest_k_dev(
            self._h, a.c_struct(), b.c_struct(), int(n_chrom), k, int(bool(signed)), md,
            idx.data_ptr() if a.n else None, dist.data_ptr() if a.n else None, self._stream()))
        return idx, dist

    # ------------------------------------------------ GROUP BY interval + SUM
    def group_rows(self, s: DeviceSide, n_chrom: int):
        """Rows with identical (chrom, raw start, raw end) share a group: returns
        ``(group_of_row int32[n], rep_row int32[n_groups])`` -- the GROUP BY half of
        count_overlaps (``intersects_duckdb.py:806-854``).  Group ids ascend with
        (chrom, start, end), the order of the linear axis, also when a genome wider
        than 32 bits is grouped by chromosomes."""
        # the kernel groups RAW coordinates (the library drops the offsets itself): so are the groups' spans taken
        raw = DeviceSide(s.chrom, s.start, s.end, 0, 0)
        return self._wide(lambda sub, _b, _rows: self._group_rows_once(sub, n_chrom),
                          lambda parts: wide.group_rows(parts, s.chrom, s.start, s.end), raw, None, n_chrom)

    def _group_rows_once(self, s: DeviceSide, n_chrom: int):
        torch = _torch()
        gid = torch.empty(s.n, dtype=torch.int32, device=self.device)
        rep = torch.empty(s.n, dtype=torch.int32, device=self.device)
        g = ctypes.c_int64(0)
        _lib.check(self._L.giql_hip_group_rows_dev(
            self._h, s.c_struct(), int(n_chrom), gid.data_ptr() if s.n else None,
            rep.data_ptr() if s.n else None, ctypes.byref(g), self._stream()))
        return gid, rep[: int(g.value)]

    def segment_sum(self, values, group_of_row, n_groups: int):
        """``sums[g] = sum(values[i] for rows i of group g)`` (int64)."""
        torch = _torch()
        if values.dtype != torch.int64 or group_of_row.dtype != torch.int32:
            raise ValueError("values must be int64 and group_of_row int32")
        n = int(values.shape[0])
        sums = torch.empty(int(n_groups), dtype=torch.int64, device=self.device)
        _lib.check(self._L.giql_hip_segment_sum_dev(
            self._h, values.data_ptr() if n else None, group_of_row.data_ptr() if n else None, n,
            sums.data_ptr() if n_groups else None, int(n_groups), self._stream()))
        return sums

    # --------------------------------------------------------- CLUSTER / MERGE
    def cluster(self, s: DeviceSide, n_chrom: int, distance: int = 0, preds=None):
        """CLUSTER ids per row (int64, 1-based within each partition ``s.chrom``):
        ``src/giql/expanders/cluster.py:210-300``.  Raw coordinates (offsets must be 0).
        ``preds`` (``predicate := ... PREV(col)``, cluster.py:281-296): ``[(lhs, op, rhs)]`` as for
        :meth:`select`, operand ``("a", column)`` = the current row's value, ``("b", column)`` = its sorted
        predecessor's; columns are device tensors of ``s.n`` rows."""
        if preds:
            return self._cluster_pred(s, n_chrom, distance, preds)
        return self._wide(lambda sub, _b, _rows: self._cluster_once(sub, n_chrom, distance),
                          lambda parts: wide.per_row(parts, s.n, self.device), s, None, n_chrom)

    @staticmethod
    def _check_pred_rows(s: DeviceSide, preds) -> None:
        for p in preds:
            for o in (p[0], p[2]):
                if o[0] in ("a", "b") and int(o[1].shape[0]) != s.n:
                    raise ValueError("a predicate column must have one value per row of the table")

    @staticmethod
    def _preds_of_rows(preds, rows):
        """CLUSTER / MERGE predicates over the rows ``rows`` of their table (one chromosome group): every
        column operand and its validity mask indexed by ``rows``; literals as they are.  ``rows=None`` is the whole
        table and no predicate stays none."""
        if not preds or rows is None:
            return preds

        def operand(o):
            if o[0] not in ("a", "b"):
                return o
            return (o[0],) + tuple(None if t is None else t[rows].contiguous() for t in o[1:])

        return [(operand(p[0]), p[1], operand(p[2])) + tuple(p[3:]) for p in preds]

    def _cluster_pred(self, s: DeviceSide, n_chrom: int, distance: int, preds):
        self._check_pred_rows(s, preds)
        return self._wide(
            lambda sub, _b, rows: self._cluster_pred_once(sub, n_chrom, distance, self._preds_of_rows(preds, rows)),
            lambda parts: wide.per_row(parts, s.n, self.device), s, None, n_chrom)

    def _cluster_pred_once(self, s: DeviceSide, n_chrom: int, distance: int, preds):
        torch = _torch()
        c_preds, k, _keep_alive, _nodes, n_nodes = self._c_preds(preds)
        if n_nodes:
            raise ValueError("arithmetic in a CLUSTER / MERGE predicate is not supported")
        ids = torch.empty(s.n, dtype=torch.int64, device=self.device)
        _lib.check(self._L.giql_hip_cluster_pred_dev(self._h, s.c_struct(), int(n_chrom), int(distance), c_preds, k,
                                                     ids.data_ptr() if s.n else None, self._stream()))
        return ids

    def _cluster_once(self, s: DeviceSide, n_chrom: int, distance: int):
        torch = _torch()
        ids = torch.empty(s.n, dtype=torch.int64, device=self.device)
        _lib.check(self._L.giql_hip_cluster_dev(self._h, s.c_struct(), int(n_chrom), int(distance),
                                                ids.data_ptr() if s.n else None, self._stream()))
        return ids

    # ---------------------------------------------------------------- DISJOIN
    def disjoin(self, target: DeviceSide, reference: DeviceSide | None = None, n_chrom: int = 0):
        """DISJOIN (``src/giql/expanders/disjoin.py:147-202``): every ``target`` row cut at the distinct starts and
        ends of ``reference`` that fall strictly inside it; a piece is kept when a reference row covers its first
        base.  ``reference=None`` is self mode (the reference is the target; every piece is kept).

        Returns ``(parent, disjoin_start, disjoin_end)`` int32 device tensors: the target row a piece was cut from
        and the piece in the TARGET's declared encoding.  Rows are ordered by parent row, then by start (the
        reference promises no order).  The row count is exact and may pass 2^31 (count, then fill, like
        :meth:`inner_plan` / :meth:`inner_fill`).  Both sides share one chromosome dictionary and need
        ``start <= end`` on every row: a ``ValueError`` names the side that does not."""
        self._check_sides(target, reference if reference is not None else target)
        return self._wide(lambda st, sr, _rows: self._disjoin_once(st, sr, n_chrom),
                          lambda parts: wide.disjoin(parts, self.device), target, reference, n_chrom)

    def _disjoin_once(self, target: DeviceSide, reference, n_chrom: int):
        torch = _torch()
        n = ctypes.c_int64(0)
        ct = target.c_struct()
        cr = reference.c_struct() if reference is not None else None
        try:
            _lib.check(self._L.giql_hip_disjoin_plan_dev(
                self._h, ctypes.byref(ct), ctypes.byref(cr) if cr is not None else None, int(n_chrom),
                ctypes.byref(n), self._stream()))
        except _lib.GiqlHipError as exc:
            if exc.code == _lib.GIQL_ERR_INVALID and "start > end" in str(exc):
                raise ValueError(str(exc)) from exc
            raise
        self._keepalive = (target, reference)
        rows = int(n.value)
        outs = [torch.empty(rows, dtype=torch.int32, device=self.device) for _ in range(3)]
        if rows:
            _lib.check(self._L.giql_hip_disjoin_fill_dev(self._h, outs[0].data_ptr(), outs[1].data_ptr(),
                                                         outs[2].data_ptr(), rows, self._stream()))
        return tuple(outs)

    # ------------------------------------------------------ coverage segments
    def coverage(self, side: DeviceSide, n_chrom: int, runs: bool = False, with_depth: bool = True):
        """Coverage profile of one table: ``SELECT disjoin_chrom, disjoin_start, disjoin_end, COUNT(*) FROM
        DISJOIN(side) GROUP BY`` the three (``bedtools genomecov -bg``, Bioconductor ``disjoin()``), computed from the
        breakpoints without DISJOIN's per-piece rows.

        Returns ``(chrom, start, end, depth)``: int32 / int32 / int32 / int64 device tensors ordered by (chrom,
        start), start and end in the side's declared encoding; ``depth`` is ``None`` with ``with_depth=False``.
        ``runs=True``: maximal runs of abutting segments of equal depth are one row each (``MERGE(interval,
        predicate := depth = PREV(depth))`` over the segments).  ``start > end`` on a row is a ``ValueError``."""
        self._check_sides(side, side)

        torch = _torch()

        def once(sub, _b, rows):
            c, st, en, d = self._coverage_once(sub, n_chrom, runs, with_depth)
            if d is None and rows is not None:  # per group: the combine orders MERGE's four columns
                d = torch.zeros(c.shape[0], dtype=torch.int64, device=self.device)
            return c, st, en, d

        out = self._wide(once, lambda parts: wide.merge(parts, self.device), side, None, n_chrom)
        return out if with_depth else out[:3] + (None,)

    def _coverage_once(self, s: DeviceSide, n_chrom: int, runs: bool, with_depth: bool):
        torch = _torch()
        cap = 2 * s.n
        c, st, en = (torch.empty(cap, dtype=torch.int32, device=self.device) for _ in range(3))
        d = torch.empty(cap if with_depth else 0, dtype=torch.int64, device=self.device)
        m = ctypes.c_int64(0)
        try:
            _lib.check(self._L.giql_hip_coverage_dev(
                self._h, s.c_struct(), int(n_chrom), _lib.COV_RUNS if runs else 0,
                c.data_ptr() if cap else None, st.data_ptr() if cap else None, en.data_ptr() if cap else None,
                d.data_ptr() if cap and with_depth else None, cap, ctypes.byref(m), self._stream()))
        except _lib.GiqlHipError as exc:
            if exc.code == _lib.GIQL_ERR_INVALID and "start > end" in str(exc):
                raise ValueError(str(exc)) from exc
            raise
        k = int(m.value)
        return c[:k], st[:k], en[:k], (d[:k] if with_depth else None)

    # ------------------------------------------------------ CONTAINS / WITHIN
    def contain_plan(self, outer: DeviceSide, inner: DeviceSide, n_chrom: int) -> int:
        self._check_sides(outer, inner)
        n = ctypes.c_int64(0)
        co, ci = outer.c_struct(), inner.c_struct()
        _lib.check(self._L.giql_hip_contain_plan_dev(self._h, ctypes.byref(co), ctypes.byref(ci), int(n_chrom),
                                                     self._stream(), ctypes.byref(n)))
        self._keepalive = (outer, inner)
        return int(n.value)

    def contain_fill(self, row_outer, row_inner) -> None:
        torch = _torch()
        cap = min(int(row_outer.shape[0]), int(row_inner.shape[0]))
        _lib.check(self._L.giql_hip_contain_fill_dev(
            self._h, self._dev_ptr(row_outer, "row_outer", torch.int32),
            self._dev_ptr(row_inner, "row_inner", torch.int32), cap, self._stream()))

    def contain_join(self, outer: DeviceSide, inner: DeviceSide, n_chrom: int):
        """All ``(row_outer, row_inner)`` with ``outer CONTAINS inner`` -- same chromosome,
        ``outer.start <= inner.start`` and ``outer.end >= inner.end`` on canonical coordinates
        (``src/giql/expanders/intersects.py:155-166``); two int32 device tensors of the exact size, pairs in no
        particular order.  ``x WITHIN y`` is ``contain_join(y, x)`` with the result columns exchanged.  Zero-length
        and inverted rows follow the literal predicate.  ``stats()["join_form"]`` tells the path: ``"uniform_b"``
        when every inner row has one length (the range of starts is exact), else ``"general"``."""
        return self._wide(lambda so, si, _rows: self._contain_once(so, si, n_chrom),
                          lambda parts: wide.pairs(parts, self.device), outer, inner, n_chrom)

    def _contain_once(self, outer: DeviceSide, inner: DeviceSide, n_chrom: int):
        torch = _torch()
        n = self.contain_plan(outer, inner, n_chrom)
        row_outer = torch.empty(n, dtype=torch.int32, device=self.device)
        row_inner = torch.empty(n, dtype=torch.int32, device=self.device)
        if n:
            self.contain_fill(row_outer, row_inner)
        return row_outer, row_inner

    # --------------------------------------------------------------- DISTANCE
    def window_join(self, a: DeviceSide, b: DeviceSide, n_chrom: int, max_distance: int):
        """All ``(row_a, row_b)`` on one chromosome with ``DISTANCE(a, b) <= max_distance`` (an integer >= 0): the
        reference's "all pairs within N bp" recipe (``docs/recipes/distance.rst:60-73``; the CASE is
        ``src/giql/expanders/_distance.py:67-117``) as the INNER join over A widened by ``max_distance``
        (``giql_hip_window_plan_dev``, filled by the INNER fill).  Overlapping rows have distance 0, book-ended
        ones 1.  Two int32 device tensors of the exact size, pairs in no particular order;
        ``stats()["join_form"]`` is always ``"general"``.  Every row of both sides needs ``start <= end``:
        :class:`InvertedRows` (a ``ValueError``) tells in ``.sides`` which side does not."""
        self._check_sides(a, b)
        max_distance = int(max_distance)
        if max_distance < 0:
            raise ValueError("max_distance must be >= 0")
        return self._wide(lambda sa, sb, _rows: self._window_once(sa, sb, n_chrom, max_distance),
                          lambda parts: wide.pairs(parts, self.device), a, b, n_chrom, pad=2)

    def _window_once(self, a: DeviceSide, b: DeviceSide, n_chrom: int, max_distance: int):
        torch = _torch()
        n = ctypes.c_int64(0)
        ca, cb = a.c_struct(), b.c_struct()
        try:
            _lib.check(self._L.giql_hip_window_plan_dev(self._h, ctypes.byref(ca), ctypes.byref(cb), int(n_chrom),
                                                        min(max_distance, (1 << 63) - 1), self._stream(),
                                                        ctypes.byref(n)))
        except _lib.GiqlHipError as exc:
            if exc.code == _lib.GIQL_ERR_INVALID:
                st = _lib.CStats()
                _lib.check(self._L.giql_hip_get_stats(self._h, ctypes.byref(st)))
                sides = tuple(s for s, v in (("a", st.n_irregular_a), ("b", st.n_irregular_b)) if int(v) == -1)
                if sides:
                    raise InvertedRows(sides, str(exc)) from exc
            raise
        self._keepalive = (a, b)
        pairs = int(n.value)
        row_a = torch.empty(pairs, dtype=torch.int32, device=self.device)
        row_b = torch.empty(pairs, dtype=torch.int32, device=self.device)
        if pairs:
            self.inner_fill(row_a, row_b)
        return row_a, row_b

    # ------------------------- SEMI / ANTI / COUNT over CONTAINS, WITHIN, DISTANCE
    _ROW_PREDICATES = {"contains": _lib.ROWPRED_CONTAINS, "within": _lib.ROWPRED_WITHIN,
                       "within_distance": _lib.ROWPRED_DISTANCE}

    def _row_predicate(self, predicate: str, max_distance):
        """``(GIQL_ROWPRED_* code, max_distance for the C call, the pad of :meth:`_groups`)``."""
        if predicate not in self._ROW_PREDICATES:
            raise ValueError(f"predicate must be one of {sorted(self._ROW_PREDICATES)}, not {predicate!r}")
        if predicate != "within_distance":
            return self._ROW_PREDICATES[predicate], 0, 0
        if max_distance is None:
            raise ValueError("within_distance needs max_distance")
        max_distance = int(max_distance)
        if max_distance < -1:
            raise ValueError("max_distance must be >= -1 (-1: `< 0`, no pair)")
        return self._ROW_PREDICATES[predicate], min(max_distance, (1 << 63) - 1), 2

    def _check_row_pred(self, rc: int) -> None:
        """:func:`_lib.check` with an inverted row under DISTANCE reported as :meth:`_window_once` reports it."""
        try:
            _lib.check(rc)
        except _lib.GiqlHipError as exc:
            if exc.code == _lib.GIQL_ERR_INVALID:
                st = _lib.CStats()
                _lib.check(self._L.giql_hip_get_stats(self._h, ctypes.byref(st)))
                sides = tuple(s for s, v in (("a", st.n_irregular_a), ("b", st.n_irregular_b)) if int(v) == -1)
                if sides:
                    raise InvertedRows(sides, str(exc)) from exc
            raise

    def semi_anti_pred(self, a: DeviceSide, b: DeviceSide, n_chrom: int, predicate: str, anti: bool,
                       max_distance=None):
        """Ascending int32 ids of the ``a`` rows with (SEMI) / without (ANTI) a ``b`` row satisfying ``predicate``:
        ``"contains"`` (a CONTAINS b), ``"within"`` (a WITHIN b) or ``"within_distance"`` (``DISTANCE(a, b) <=
        max_distance``; -1 stands for ``< 0`` and selects no pair).  Exactly the left rows of :meth:`contain_join` /
        :meth:`window_join` (``giql_hip_semi_anti_pred_dev``: one sort of ``b``, one prefix maximum, one binary
        search per row -- no pair is written).  Zero-length rows follow the literal predicate, inverted rows too
        under containment; DISTANCE raises :class:`InvertedRows` for them."""
        self._check_sides(a, b)
        code, md, pad = self._row_predicate(predicate, max_distance)
        return self._wide(lambda sa, sb, _rows: self._semi_anti_pred_once(sa, sb, n_chrom, code, md, anti),
                          lambda parts: wide.row_ids(parts, self.device), a, b, n_chrom, pad=pad)

    def _semi_anti_pred_once(self, a: DeviceSide, b: DeviceSide, n_chrom: int, code: int, md: int, anti: bool):
        torch = _torch()
        rows = torch.empty(a.n, dtype=torch.int32, device=self.device)
        n = ctypes.c_int64(0)
        self._check_row_pred(self._L.giql_hip_semi_anti_pred_dev(
            self._h, a.c_struct(), b.c_struct(), int(n_chrom), code, md, int(bool(anti)),
            rows.data_ptr() if a.n else None, ctypes.byref(n), self._stream()))
        return rows[: int(n.value)]

    def count_pred(self, a: DeviceSide, b: DeviceSide, n_chrom: int, predicate: str, max_distance=None):
        """int64 tensor: the number of ``b`` rows satisfying ``predicate`` per ``a`` row, in ``a``'s order (the
        predicates of :meth:`semi_anti_pred`; ``giql_hip_count_pred_dev``).  DISTANCE is a rank difference over two
        sorts of ``b``; containment walks the CONTAINS plan's candidate tiles and adds per row --
        ``stats()["join_form"]`` is ``"uniform_b"`` when ``b`` has one length under ``"contains"`` (its range counts
        are exact), else ``"general"``."""
        self._check_sides(a, b)
        code, md, pad = self._row_predicate(predicate, max_distance)
        return self._wide(lambda sa, sb, _rows: self._count_pred_once(sa, sb, n_chrom, code, md),
                          lambda parts: wide.per_row(parts, a.n, self.device), a, b, n_chrom, pad=pad)

    def _count_pred_once(self, a: DeviceSide, b: DeviceSide, n_chrom: int, code: int, md: int):
        torch = _torch()
        # (no pre-fill: the library writes every slot -- its own memset where the tile walk adds into the counts)
        counts = torch.empty(a.n, dtype=torch.int64, device=self.device)
        self._check_row_pred(self._L.giql_hip_count_pred_dev(
            self._h, a.c_struct(), b.c_struct(), int(n_chrom), code, md,
            counts.data_ptr() if a.n else None, self._stream()))
        return counts

    def distance(self, a: DeviceSide, b: DeviceSide, row_a, row_b, signed: bool = False, stranded: bool = False,
                 strand_a=None, strand_b=None):
        """``DISTANCE(a[row_a[i]], b[row_b[i]])`` per pair: ``(distance int64, valid uint8)`` device tensors, the
        four variants of ``src/giql/expanders/_distance.py:67-117``.  ``valid == 0`` is SQL NULL (the chromosomes
        differ; stranded: a strand is NULL / ``.`` / ``?``).  ``strand_a`` / ``strand_b``: int32 device tensors,
        one code per table row as ``execute._strand_codes`` makes them (0 ``+``, 1 ``-``, 2 ``.``, 3 ``?``, other =
        NULL); required when ``stranded``.  Row ids outside their table raise ``GiqlHipError``."""
        torch = _torch()
        self._check_sides(a, b)
        n = int(row_a.shape[0])
        if int(row_b.shape[0]) != n:
            raise ValueError("row_a and row_b must have one entry per pair")
        flags = (1 if signed else 0) | (2 if stranded else 0)
        if stranded:
            for s, side, what in ((strand_a, a, "strand_a"), (strand_b, b, "strand_b")):
                if s is None or int(s.shape[0]) != side.n:
                    raise ValueError(f"stranded DISTANCE needs {what}: one int32 code per row of its table")
        dist = torch.empty(n, dtype=torch.int64, device=self.device)
        valid = torch.empty(n, dtype=torch.uint8, device=self.device)
        ca, cb = a.c_struct(), b.c_struct()
        _lib.check(self._L.giql_hip_distance_dev(
            self._h, ctypes.byref(ca), ctypes.byref(cb), self._dev_ptr(row_a, "row_a", torch.int32),
            self._dev_ptr(row_b, "row_b", torch.int32), n,
            self._dev_ptr(strand_a, "strand_a", torch.int32) if stranded else None,
            self._dev_ptr(strand_b, "strand_b", torch.int32) if stranded else None,
            flags, dist.data_ptr() if n else None, valid.data_ptr() if n else None, self._stream()))
        return dist, valid

    def merge(self, s: DeviceSide, n_chrom: int, distance: int = 0, preds=None):
        """MERGE: ``(chrom, start, end, count)`` tensors of the merged regions ordered by
        (chrom, start) (``src/giql/expanders/merge.py:186-330``).  ``preds``: the ``predicate :=``
        argument, as for :meth:`cluster` (merge.py:201-210 hands it to the CLUSTER underneath)."""
        if preds:
            self._check_pred_rows(s, preds)
        return self._wide(
            lambda sub, _b, rows: self._merge_once(sub, n_chrom, distance, self._preds_of_rows(preds, rows)),
            lambda parts: wide.merge(parts, self.device), s, None, n_chrom)

    def _merge_once(self, s: DeviceSide, n_chrom: int, distance: int, preds=None):
        torch = _torch()
        n = s.n
        c = torch.empty(n, dtype=torch.int32, device=self.device)
        st = torch.empty(n, dtype=torch.int32, device=self.device)
        en = torch.empty(n, dtype=torch.int32, device=self.device)
        cnt = torch.empty(n, dtype=torch.int64, device=self.device)
        m = ctypes.c_int64(0)
        outs = (c.data_ptr() if n else None, st.data_ptr() if n else None, en.data_ptr() if n else None,
                cnt.data_ptr() if n else None, n, ctypes.byref(m), self._stream())
        if preds:
            c_preds, k, _keep_alive, _nodes, n_nodes = self._c_preds(preds)
            if n_nodes:
                raise ValueError("arithmetic in a CLUSTER / MERGE predicate is not supported")
            _lib.check(self._L.giql_hip_merge_pred_dev(self._h, s.c_struct(), int(n_chrom), int(distance), c_preds, k,
                                                       *outs))
        else:
            _lib.check(self._L.giql_hip_merge_dev(self._h, s.c_struct(), int(n_chrom), int(distance), *outs))
        k = int(m.value)
        return c[:k], st[:k], en[:k], cnt[:k]

    #: aggregates per :meth:`merge_agg` call, as asked for (the C ABI takes 8 kernel aggregates)
    MERGE_AGG_MAX = 8
    #: STRING_AGG entries per :meth:`merge_agg` call (``GIQL_STR_AGG_MAX``)
    MERGE_STR_AGG_MAX = _lib.STR_AGG_MAX

    @staticmethod
    def _check_agg_column(func: str, t, valid, n: int, table: str, validity_of: str) -> None:
        """A numeric entry of :meth:`merge_agg` / :meth:`pair_aggregate` over a table of ``n`` rows; ``table`` and
        ``validity_of`` word the two messages.  ``t`` may be ``None`` where the caller allows it."""
        torch = _torch()
        if func not in ("COUNT", "SUM", "MIN", "MAX", "AVG"):
            raise ValueError(f"aggregate function {func!r}")
        if t is not None and (t.dtype not in (torch.int32, torch.int64, torch.float32, torch.float64) or t.dim() != 1
                              or not t.is_contiguous() or int(t.shape[0]) != n):
            raise ValueError("an aggregate column must be a contiguous 1-D int32/int64/float32/float64 tensor "
                             f"with one value per row of the {table}")
        if valid is not None and (valid.dtype not in (torch.uint8, torch.bool) or valid.dim() != 1
                                  or int(valid.shape[0]) != n or not valid.is_contiguous()):
            raise ValueError(f"validity must be a contiguous uint8/bool tensor of {validity_of}")

    def merge_agg(self, s: DeviceSide, n_chrom: int, distance: int, aggs, preds=None):
        """MERGE with aggregates per merged region (``src/giql/expanders/merge.py:317-390``): the four tensors of
        :meth:`merge` plus, per entry of ``aggs``, ``(values, valid)``.  An entry is ``(func, values_tensor,
        valid_tensor_or_None)``, ``func`` in COUNT, SUM, MIN, MAX, AVG; the tensors are contiguous int32 / int64 /
        float32 / float64 (validity: uint8 / bool) device tensors of ``s.n`` rows.  ``valid`` is "the region has a
        non-NULL input" (COUNT: always).  SUM / MIN / MAX of an integer column are int64, of a float column float64;
        AVG is ``double(sum) / double(non-NULL count)`` computed on the device from the kernel's SUM, which a SUM
        over the same column shares.  Float sums use no atomics: the same call returns the same bits.

        An entry ``("STRING_AGG", offsets, data, valid_or_None, separator)`` joins a string column -- Arrow utf8 as
        contiguous device tensors, int32 ``offsets`` of ``s.n + 1`` entries and uint8 ``data`` -- per region
        (bedtools ``merge -o collapse``; ``giql_hip_merge_str_dev``): its result is ``(out_offsets, out_data, valid)``,
        the utf8 layout of one string per region.  NULL rows are skipped, a region with no non-NULL row is NULL, an
        empty string is a value; the members are joined in ascending start, then row order.  ``separator``: ``str``
        or ``bytes`` of at most 255 bytes.  At most :attr:`MERGE_STR_AGG_MAX` such entries, and 2^31 - 1 bytes of
        output each (``GIQL_ERR_CAPACITY`` past that).  A call without such an entry is ``giql_hip_merge_agg_dev``'s."""
        torch = _torch()
        entries = []   # (func, values, valid) | ("STRING_AGG", offsets, data, valid, separator bytes)
        for a in aggs:
            func = str(a[0]).upper()
            if func != "STRING_AGG":
                entries.append((func, a[1], a[2] if len(a) > 2 else None))
                continue
            if len(a) != 5:
                raise ValueError("a STRING_AGG entry is (\"STRING_AGG\", offsets, data, valid_or_None, separator)")
            _f, off, data, valid, sep = a
            sep = sep.encode("utf-8") if isinstance(sep, str) else bytes(sep)
            if len(sep) > _lib.STR_AGG_MAX_SEP:
                raise ValueError(f"STRING_AGG separator of {len(sep)} bytes: at most {_lib.STR_AGG_MAX_SEP}")
            if (off.dtype != torch.int32 or off.dim() != 1 or not off.is_contiguous() or int(off.shape[0]) != s.n + 1
                    or data.dtype != torch.uint8 or data.dim() != 1 or not data.is_contiguous()):
                raise ValueError("a STRING_AGG column is contiguous int32 offsets of one entry per row plus one, and "
                                 "contiguous uint8 data")
            self._check_agg_column("COUNT", None, valid, s.n, "table", "the column's length")
            entries.append((func, off, data, valid, sep))
        n_str = sum(e[0] == "STRING_AGG" for e in entries)
        if not n_str and not 1 <= len(entries) <= self.MERGE_AGG_MAX:
            raise ValueError(f"MERGE takes 1 to {self.MERGE_AGG_MAX} aggregates, got {len(entries)}")
        if len(entries) > self.MERGE_AGG_MAX or n_str > self.MERGE_STR_AGG_MAX:
            raise ValueError(f"MERGE takes at most {self.MERGE_AGG_MAX} aggregates, {self.MERGE_STR_AGG_MAX} of them "
                             f"STRING_AGG; got {len(entries)} and {n_str}")
        for e in entries:
            if e[0] != "STRING_AGG":
                self._check_agg_column(*e, s.n, "table", "the column's length")
        if preds:
            self._check_pred_rows(s, preds)
        dtypes = [wide.UTF8 if e[0] == "STRING_AGG" else
                  torch.float64 if e[0] == "AVG" or (e[0] != "COUNT" and e[1].is_floating_point()) else torch.int64
                  for e in entries]

        def of_rows(rows):
            if rows is None:
                return entries
            taken = {}   # one copy per tensor / string column: aggregates over one column keep sharing it

            def take(t):
                if t is not None and t.data_ptr() not in taken:
                    taken[t.data_ptr()] = t[rows].contiguous()
                return None if t is None else taken[t.data_ptr()]

            def take_str(off, data):
                key = (off.data_ptr(), data.data_ptr())
                if key not in taken:
                    taken[key] = self.take_utf8(off, data, rows.to(torch.int32).contiguous())
                return taken[key]

            return [(e[0],) + take_str(e[1], e[2]) + (take(e[3]), e[4]) if e[0] == "STRING_AGG"
                    else (e[0], take(e[1]), take(e[2])) for e in entries]

        return self._wide(
            lambda sub, _b, rows: self._merge_agg_once(sub, n_chrom, distance, of_rows(rows),
                                                       self._preds_of_rows(preds, rows)),
            lambda parts: wide.merge_agg(parts, self.device, dtypes), s, None, n_chrom)

    def _kernel_aggs(self, entries, n_out: int, ctype=_lib.CAgg):
        """The kernel's aggregates for the entries ``(func, key, source)`` of one call, ``n_out`` outputs each: AVG
        asks for SUM, and entries of equal function and ``key`` -- the caller's name for the source: a column, a
        validity alone, an expression program -- share one.  ``source``: ``("col", values_or_None, valid_or_None)`` or
        ``("expr", first node, nodes, can_float)``.  Returns ``(array of ctype, [(out, non_null)], slot per entry)``."""
        torch = _torch()
        types = {torch.int32: _lib.T_I32, torch.int64: _lib.T_I64, torch.float32: _lib.T_F32,
                 torch.float64: _lib.T_F64}
        kernel, slot = {}, []
        for func, key, src in entries:
            key = ("SUM" if func == "AVG" else func, key)
            if key not in kernel:
                flt = key[0] != "COUNT" and (src[3] if src[0] == "expr" else src[1] is not None and src[1].is_floating_point())
                kernel[key] = (src, torch.empty(n_out, dtype=torch.float64 if flt else torch.int64, device=self.device),
                               torch.empty(n_out, dtype=torch.int64, device=self.device))
            slot.append(list(kernel).index(key))
        c_aggs = (ctype * max(len(kernel), 1))()
        for c, (key, (src, out, nn)) in zip(c_aggs, kernel.items()):
            c.func = _lib.AGG_FUNCS[key[0]]
            if src[0] == "expr":
                c.first, c.count, c.type = src[1], src[2], _lib.T_F64 if src[3] else _lib.T_I64
            else:
                c.type = _lib.T_I32 if src[1] is None else types[src[1].dtype]
                c.data = self._dev_ptr(src[1], "an aggregate column")
                if src[1] is not None and c.data is None:
                    c.data = 1  # (a table without rows: never dereferenced)
                c.valid = self._dev_ptr(src[2], "a validity column")
            c.out = out.data_ptr() if n_out else 1
            c.out_nn = nn.data_ptr() if n_out else None
        return c_aggs, [(out, nn) for _src, out, nn in kernel.values()], slot

    @staticmethod
    def _agg_value(func: str, out, nn):
        """An entry's values from its kernel aggregate: AVG is ``double(sum) / double(non_null)``; NULL reads 0."""
        torch = _torch()
        if func != "AVG":
            return out
        return torch.where(nn > 0, out.double() / nn.double(), torch.zeros(out.shape[0], dtype=torch.float64, device=out.device))

    def _merge_agg_once(self, s: DeviceSide, n_chrom: int, distance: int, entries, preds=None):
        """One library call of :meth:`merge_agg` over its checked entries: ``giql_hip_merge_str_dev`` and one fill per
        string where there is a STRING_AGG entry, else ``giql_hip_merge_agg_dev``."""
        torch = _torch()
        n = s.n
        nums = [e for e in entries if e[0] != "STRING_AGG"]
        strs = [e for e in entries if e[0] == "STRING_AGG"]
        c_aggs, kernel, slot = self._kernel_aggs(
            [(f, (t.data_ptr(), None if v is None else v.data_ptr(), t.dtype), ("col", t, v)) for f, t, v in nums], n)
        c_strs = (_lib.CStrAgg * len(strs))()
        str_outs = []
        for cs, (_f, off, _data, valid, sep) in zip(c_strs, strs):
            out_off = torch.empty(n + 1, dtype=torch.int32, device=self.device)
            nn = torch.empty(max(n, 1), dtype=torch.int64, device=self.device)
            row_dst = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)  # (uint32 words)
            str_outs.append((out_off, nn, row_dst))
            cs.offsets = off.data_ptr()
            cs.valid = valid.data_ptr() if valid is not None and n else None
            cs.sep_len = len(sep)
            cs.out_offsets, cs.out_nn, cs.row_dst = out_off.data_ptr(), nn.data_ptr(), row_dst.data_ptr()
        c = torch.empty(n, dtype=torch.int32, device=self.device)
        st = torch.empty(n, dtype=torch.int32, device=self.device)
        en = torch.empty(n, dtype=torch.int32, device=self.device)
        cnt = torch.empty(n, dtype=torch.int64, device=self.device)
        m = ctypes.c_int64(0)
        c_preds, k = None, 0
        if preds:
            c_preds, k, _keep_alive, _nodes, n_nodes = self._c_preds(preds)
            if n_nodes:
                raise ValueError("arithmetic in a CLUSTER / MERGE predicate is not supported")
        head = (self._h, s.c_struct(), int(n_chrom), int(distance), c_preds, k, c_aggs if nums else None, len(kernel))
        rows = (c.data_ptr() if n else None, st.data_ptr() if n else None, en.data_ptr() if n else None,
                cnt.data_ptr() if n else None)
        if strs:
            order = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
            _lib.check(self._L.giql_hip_merge_str_dev(*head, c_strs, len(strs), *rows, order.data_ptr(), n,
                                                      ctypes.byref(m), self._stream()))
        else:
            _lib.check(self._L.giql_hip_merge_agg_dev(*head, *rows, n, ctypes.byref(m), self._stream()))
        r = int(m.value)
        num_res = []
        for (func, _t, _v), j in zip(nums, slot):
            out, nn = kernel[j][0][:r], kernel[j][1][:r]
            if func == "COUNT":
                num_res.append((out, torch.ones(r, dtype=torch.bool, device=self.device)))
                continue
            out = self._agg_value(func, out, nn)
            num_res.append((torch.where(nn > 0, out, torch.zeros_like(out)), nn > 0))
        str_res = []
        for cs, (out_off, nn, row_dst), (_f, off, data, _valid, sep) in zip(c_strs, str_outs, strs):
            out = torch.empty(int(cs.n_bytes), dtype=torch.uint8, device=self.device)
            if out.numel():
                _lib.check(self._L.giql_hip_concat_utf8_fill_dev(
                    self._h, off.data_ptr(), data.data_ptr() if data.numel() else None, n, order.data_ptr(),
                    row_dst.data_ptr(), n, sep, len(sep), out.data_ptr(), self._stream()))
            str_res.append((out_off[: r + 1], out, nn[:r] > 0))
        num_res, str_res = iter(num_res), iter(str_res)
        return (c[:r], st[:r], en[:r], cnt[:r]) + tuple(next(str_res if e[0] == "STRING_AGG" else num_res)
                                                        for e in entries)

    #: aggregates per :meth:`pair_aggregate` call, as asked for (``GIQL_PAIR_AGG_MAX`` kernel aggregates)
    PAIR_AGG_MAX = 8

    def pair_aggregate(self, row_a, row_b, n_a: int, n_b: int, aggs):
        """Aggregates over a join's pairs per left row (``giql_hip_pair_agg_dev``; bedtools ``map``): ``row_a`` /
        ``row_b`` are the int32 device pair arrays of a join of ``n_a`` x ``n_b`` rows, in any order.  ``aggs`` takes
        the tuples of :meth:`merge_agg` -- ``(func, values, valid_or_None)`` with ``func`` in COUNT, SUM, MIN, MAX,
        AVG -- over columns of ``n_b`` rows; a COUNT may give ``None`` for ``values`` (it reads validity alone, so
        ``COUNT(b.name)`` needs no numeric column).

        Returns ``(pairs, results)``: ``pairs`` the int64 pair count of every A row, ``results`` one ``(values,
        non_null)`` per entry, both of ``n_a`` rows in A's order; ``non_null`` is the int64 number of non-NULL inputs
        (0: the value is NULL and reads 0).  SUM / MIN / MAX of an integer column are int64, of a float column
        float64; AVG is ``double(sum) / double(non_null)``; COUNT is ``non_null``.  A row's values are reduced in
        ascending ``row_b`` without atomics: the result does not depend on the order of the pairs, float sums
        included.  Ids outside their table raise ``GiqlHipError``.

        In place of the values tensor an entry may give ``("expr", tree)``: the aggregate of an EXPRESSION evaluated at
        every pair (``giql_hip_pair_expr_agg_dev``), ``tree`` being what :meth:`eval_exprs` takes, ``("if", ...)`` and
        ``("null",)`` included; its ``"a"`` columns hold ``n_a`` rows, its ``"b"`` columns ``n_b``.  A pair at which
        the tree is NULL is no input.  SUM / MIN / MAX are float64 where :func:`expr_can_float` says the tree can
        yield a float, else int64.  The values are reduced as they are computed: no per-pair array is made.  A call
        takes at most 256 expression nodes in total; a call without such an entry is ``giql_hip_pair_agg_dev``'s."""
        torch = _torch()
        aggs = [(str(a[0]).upper(), a[1], a[2] if len(a) > 2 else None) for a in aggs]
        n_a, n_b = int(n_a), int(n_b)
        if len(aggs) > self.PAIR_AGG_MAX:
            raise ValueError(f"a pair aggregate takes at most {self.PAIR_AGG_MAX} aggregates, got {len(aggs)}")
        n = int(row_a.shape[0])
        if int(row_b.shape[0]) != n or row_a.dim() != 1 or row_b.dim() != 1:
            raise ValueError("row_a and row_b must have one entry per pair")
        nodes, keep_alive, progs = [], [], {}   # progs: tree key -> (first, count, can_float)
        entries = []
        for func, t, valid in aggs:
            if isinstance(t, tuple):
                self._check_agg_column(func, None, None, n_b, "", "")
                if len(t) != 2 or t[0] != "expr":
                    raise ValueError('an expression source is ("expr", tree)')
                if valid is not None:
                    raise ValueError("an expression source takes no validity column: its tree names them")
                tkey = self._expr_key(t[1], n_a, n_b)
                if tkey not in progs:
                    first = len(nodes)
                    self._flatten_expr(t[1], nodes, keep_alive)
                    progs[tkey] = (first, len(nodes) - first, expr_can_float(t[1]))
                entries.append((func, ("expr", tkey), ("expr",) + progs[tkey]))
                continue
            if func in ("SUM", "MIN", "MAX", "AVG") and t is None:
                raise ValueError(f"{func} needs a values tensor (only COUNT reads validity alone)")
            self._check_agg_column(func, t, valid, n_b, "right table", "one entry per right row")
            vkey = None if valid is None else valid.data_ptr()
            if func == "COUNT":  # COUNT reads validity alone: every COUNT over one validity shares
                entries.append((func, (None, vkey, None), ("col", None, valid)))
            else:
                entries.append((func, (t.data_ptr(), vkey, t.dtype), ("col", t, valid)))
        if len(nodes) > 256:
            raise ValueError(f"a pair aggregate takes at most 256 expression nodes per call, got {len(nodes)}")
        c_aggs, kernel, slot = self._kernel_aggs(entries, n_a, _lib.CPairExprAgg if progs else _lib.CAgg)
        pairs = torch.empty(n_a, dtype=torch.int64, device=self.device)
        rows = (self._h, self._dev_ptr(row_a, "row_a", torch.int32), self._dev_ptr(row_b, "row_b", torch.int32), n,
                n_a, n_b)
        tail = (c_aggs, len(kernel), pairs.data_ptr() if n_a else None, self._stream())
        if progs:
            c_nodes = (_lib.COperand * len(nodes))(*nodes)
            _lib.check(self._L.giql_hip_pair_expr_agg_dev(*rows, c_nodes, len(nodes), *tail))
        else:
            _lib.check(self._L.giql_hip_pair_agg_dev(*rows, *tail))
        return pairs, [(self._agg_value(func, *kernel[j]), kernel[j][1]) for (func, _t, _v), j in zip(aggs, slot)]

    def _expr_key(self, tree, n_a: int, n_b: int):
        """A hashable restatement of ``tree`` (columns by address): equal keys are one program.  Checks every column's
        row count against its table on the way -- the kernel reads a column at the pair's row id."""
        kind = tree[0]
        if kind in ("a", "b"):
            t, valid = tree[1], tree[2] if len(tree) > 2 else None
            if int(t.shape[0]) != (n_a if kind == "a" else n_b):
                raise ValueError(f"a column of side {kind!r} must have one value per row of its table")
            return (kind, t.data_ptr(), str(t.dtype), None if valid is None else valid.data_ptr())
        if kind == "lit":
            return ("lit", type(tree[1]).__name__, tree[1])
        return (kind,) + tuple(self._expr_key(c, n_a, n_b) for c in tree[1:])

    # ------------------------------------------------------------- projection
    def take(self, cols, idx, outs=None):
        """Arrow ``take`` of fixed-width device columns by int32 row ids ``idx``
        (the reference's outer SELECT, ``intersects_duckdb.py:1402-1644``); one
        fused launch per 8 columns.  ``idx < 0`` yields zeros.  Returns new tensors,
        or fills the caller's ``outs`` (contiguous, same dtype, ``len(idx)`` rows)."""
        torch = _torch()
        cols = list(cols)
        if idx.dtype != torch.int32 or not idx.is_contiguous():
            raise ValueError("idx must be a contiguous int32 tensor")
        n = int(idx.shape[0])
        n_rows = int(cols[0].shape[0]) if cols else 0
        given = None if outs is None else list(outs)
        if given is not None and len(given) != len(cols):
            raise ValueError("outs must match cols")
        outs = []
        for k, c in enumerate(cols):
            if c.dim() != 1 or not c.is_contiguous() or int(c.shape[0]) != n_rows:
                raise ValueError("columns must be contiguous 1-D tensors of equal length")
            if c.device != idx.device:
                raise ValueError("columns and idx must live on the same device")
            if given is None:
                outs.append(torch.empty(n, dtype=c.dtype, device=c.device))
            else:
                o = given[k]
                if (o.dtype != c.dtype or o.device != c.device or o.dim() != 1 or int(o.shape[0]) != n
                        or not o.is_contiguous()):
                    raise ValueError("outs[k] must be a contiguous 1-D tensor of len(idx) rows and the column's dtype")
                outs.append(o)
        k = len(cols)
        if k == 0 or n == 0:
            return outs
        vp = ctypes.c_void_p
        c_cols = (vp * k)(*[c.data_ptr() if n_rows else None for c in cols])
        c_outs = (vp * k)(*[o.data_ptr() for o in outs])
        c_elem = (ctypes.c_int32 * k)(*[c.element_size() for c in cols])
        _lib.check(self._L.giql_hip_take_dev(self._h, c_cols, c_elem, k, n_rows, idx.data_ptr(), n,
                                             c_outs, self._stream()))
        return outs

    def take_utf8(self, offsets, data, idx):
        """``take`` of an Arrow utf8/binary column held as device tensors: int32
        ``offsets[n_rows + 1]`` and uint8 ``data``.  Returns ``(out_offsets, out_data)``.
        One call takes at most 0x7FFFFFF0 ids and 0x7FFFFFFF gathered bytes (int32 output
        offsets): past either it raises ``GiqlHipError``; ``execute`` splits such a gather
        by rows (``execute.plan_utf8_slices``)."""
        torch = _torch()
        if offsets.dtype != torch.int32 or data.dtype != torch.uint8 or idx.dtype != torch.int32:
            raise ValueError("offsets/idx must be int32 and data uint8")
        n = int(idx.shape[0])
        n_rows = int(offsets.shape[0]) - 1
        if n_rows < 0:
            raise ValueError("offsets must hold n_rows + 1 entries")
        out_off = torch.empty(n + 1, dtype=torch.int32, device=idx.device)
        nbytes = ctypes.c_int64(0)
        _lib.check(self._L.giql_hip_take_utf8_plan_dev(
            self._h, offsets.data_ptr(), n_rows, idx.data_ptr() if n else None, n, out_off.data_ptr(),
            ctypes.byref(nbytes), self._stream()))
        out = torch.empty(int(nbytes.value), dtype=torch.uint8, device=idx.device)
        if nbytes.value:
            _lib.check(self._L.giql_hip_take_utf8_fill_dev(
                self._h, offsets.data_ptr(), data.data_ptr() if data.numel() else None, n_rows,
                idx.data_ptr(), n, out_off.data_ptr(), out.data_ptr(), self._stream()))
        return out_off, out

    # ----------------------------------------------------- residual predicates
    _XOPS = {"+": 16, "-": 17, "*": 18, "/": 19, "neg": 20, "abs": 21, "least": 22, "greatest": 23,
             # boolean nodes (three-valued): a whole condition as one program, GIQL_X_EQ .. GIQL_X_NOT
             "=": 24, "!=": 25, "<": 26, "<=": 27, ">": 28, ">=": 29, "isnull": 30, "notnull": 31,
             "and": 32, "or": 33, "not": 34}
    _UNARY = ("neg", "abs", "isnull", "notnull", "not")
    _NARY = ("least", "greatest", "and", "or")

    def _flatten_expr(self, tree, nodes, keep_alive) -> None:
        """Append the postfix form of ``tree`` -- ``("a" | "b", column[, valid])``, ``("lit", v)`` or
        ``(op, child, ...)`` with op one of ``+ - * / neg abs least greatest``, a comparison, ``isnull`` /
        ``notnull``, ``and`` / ``or`` / ``not``; ``("if", cond, then, else)`` and ``("null",)`` (a searched CASE and
        its missing ELSE: GIQL_X_IF / GIQL_X_NULL) -- to ``nodes``."""
        kind = tree[0]
        if kind in ("a", "b", "lit"):
            o, ka = self._c_operand(tree)
            nodes.append(o)
            keep_alive.append(ka)
            return
        if kind in ("if", "null"):
            if len(tree) != (4 if kind == "if" else 1):
                raise ValueError(f"{kind!r} with {len(tree) - 1} argument(s)")
            for child in tree[1:]:
                self._flatten_expr(child, nodes, keep_alive)
            nd = _lib.COperand()
            nd.side = _lib.X_IF if kind == "if" else _lib.X_NULL
            nodes.append(nd)
            return
        if kind not in self._XOPS:
            raise ValueError(f"expression operator {kind!r}")
        args = tree[1:]
        arity_ok = (len(args) == 1) if kind in self._UNARY else (len(args) >= 1 if kind in self._NARY
                                                                  else len(args) == 2)
        if not arity_ok:
            raise ValueError(f"{kind!r} with {len(args)} argument(s)")
        self._flatten_expr(args[0], nodes, keep_alive)
        op = _lib.COperand()
        op.side = self._XOPS[kind]
        if kind in self._UNARY:
            nodes.append(op)
            return
        for child in args[1:]:
            self._flatten_expr(child, nodes, keep_alive)
            nd = _lib.COperand()
            nd.side = op.side
            nodes.append(nd)

    def _c_preds(self, preds):
        """``[(lhs, op, rhs[, group])]`` -> (``giql_pred`` array, its length, the tensors to keep alive, the
        expression nodes as a ``giql_operand`` array, their number).  Predicates are AND-ed; adjacent ones
        sharing a non-zero ``group`` are OR-ed (one CNF clause).  An operand ``("expr", tree)`` is arithmetic
        over columns and literals (``giql_hip_select_expr_dev``)."""
        k = len(preds)
        if k > 16:
            raise ValueError("at most 16 predicates per call")
        c_preds = (_lib.CPred * max(k, 1))()
        keep_alive, nodes = [], []

        def operand(spec):
            if spec[0] != "expr":
                return self._c_operand(spec)
            first = len(nodes)
            self._flatten_expr(spec[1], nodes, keep_alive)
            o = _lib.COperand()
            o.side, o.lit_i, o.type = _lib.SIDE_EXPR, first, len(nodes) - first
            return o, ()

        for j, p in enumerate(preds):
            lhs, op, rhs = p[0], p[1], p[2]
            if op not in _lib.OPS:
                raise ValueError(f"operator {op!r}")
            c_preds[j].lhs, ka = operand(lhs)
            keep_alive.append(ka)
            c_preds[j].rhs, ka = operand(rhs if op not in ("isnull", "notnull", "istrue") else ("lit", 0))
            keep_alive.append(ka)
            c_preds[j].op = _lib.OPS[op]
            c_preds[j].group = int(p[3]) if len(p) > 3 else 0
        if len(nodes) > 256:
            raise ValueError("at most 256 expression nodes per call")
        c_nodes = (_lib.COperand * max(len(nodes), 1))(*nodes)
        return c_preds, k, keep_alive, c_nodes, len(nodes)

    def _c_operand(self, spec):
        """``("a" | "b", tensor[, valid_u8_tensor])`` or ``("lit", int | float)`` -> COperand."""
        torch = _torch()
        o = _lib.COperand()
        if spec[0] == "lit":
            o.side = _lib.SIDE_LIT
            v = spec[1]
            if isinstance(v, bool):
                v = int(v)
            if isinstance(v, int):
                if not -(2**63) <= v < 2**63:
                    raise ValueError("integer literal does not fit int64")
                o.lit_i, o.lit_is_float = v, 0
            elif isinstance(v, float):
                o.lit_f, o.lit_is_float = v, 1
            else:
                raise ValueError(f"unsupported literal {v!r}")
            return o, ()
        if spec[0] not in ("a", "b"):
            raise ValueError(f"operand side {spec[0]!r}")
        t = spec[1]
        types = {torch.int32: _lib.T_I32, torch.int64: _lib.T_I64, torch.float32: _lib.T_F32,
                 torch.float64: _lib.T_F64, torch.uint8: _lib.T_U8, torch.bool: _lib.T_U8}
        if t.dtype not in types or t.dim() != 1 or not t.is_contiguous():
            raise ValueError("predicate columns must be contiguous 1-D int32/int64/float32/float64/uint8 tensors")
        o.side = _lib.SIDE_A if spec[0] == "a" else _lib.SIDE_B
        o.type = types[t.dtype]
        o.data = t.data_ptr() if t.numel() else 1  # never dereferenced when empty
        valid = spec[2] if len(spec) > 2 else None
        if valid is not None:
            if valid.dtype not in (torch.uint8, torch.bool) or valid.shape != t.shape or not valid.is_contiguous():
                raise ValueError("validity must be a contiguous uint8/bool tensor of the column's length")
            o.valid = valid.data_ptr() if valid.numel() else None
        return o, (t, valid)

    #: candidates per ``giql_hip_select_expr_dev`` call; the C ABI takes at most 0x7FFFFFF0
    SELECT_SLICE = 1 << 30

    def select(self, preds, idx_a=None, idx_b=None, n=None, n_rows_a=0, n_rows_b=0, want=("a", "b")):
        """Stable filter by residual predicates (the extra ON / WHERE conditions the
        reference inlines beside the INTERSECTS, ``intersects_duckdb.py:1164-1177,
        1239-1243``), given in conjunctive normal form.

        ``preds`` = ``[(lhs, op, rhs[, group])]`` with operands ``("a" | "b", column[, valid])``
        or ``("lit", value)`` and ``op`` one of ``= != <> < <= > >= isnull notnull``; the
        predicates are AND-ed, adjacent ones sharing a non-zero ``group`` are OR-ed.  Candidates are the
        pairs ``(idx_a[i], idx_b[i])``; a missing id array means "the candidate index".
        Returns the kept ``(ids_a, ids_b)`` (``None`` for a side not in ``want``).

        Any ``n`` is accepted: the C ABI takes at most 0x7FFFFFF0 candidates per call, so they
        are filtered in slices of :attr:`SELECT_SLICE`, each slice's kept ids written straight
        after the previous slice's into the one output.  A slice past the first addresses a
        side without an id array through ``arange(lo, hi)``: the candidate index stays global."""
        torch = _torch()
        if n is None:
            n = int((idx_a if idx_a is not None else idx_b).shape[0])
        n = int(n)
        c_preds, k, _keep_alive, c_nodes, n_nodes = self._c_preds(preds)
        for t in (idx_a, idx_b):
            if t is not None and (t.dtype != torch.int32 or not t.is_contiguous() or int(t.shape[0]) != n):
                raise ValueError("id arrays must be contiguous int32 tensors of n rows")
        out_a = torch.empty(n, dtype=torch.int32, device=self.device) if "a" in want else None
        out_b = torch.empty(n, dtype=torch.int32, device=self.device) if "b" in want else None
        m = 0
        for lo in range(0, max(n, 1), self.SELECT_SLICE):
            hi = min(n, lo + self.SELECT_SLICE)
            ids, rows = [], []
            for t, n_rows in ((idx_a, int(n_rows_a)), (idx_b, int(n_rows_b))):
                if t is not None:
                    t = t[lo:hi]
                elif lo:
                    # the first slice has checked a side addressed by the candidate index against its
                    # row count: a used side with n_rows 0 has failed there, so 0 here means "unused"
                    t = torch.arange(lo, hi, dtype=torch.int32, device=self.device)
                    n_rows = n_rows or n
                ids.append(t)
                rows.append(n_rows)
            kept = ctypes.c_int64(0)
            _lib.check(self._L.giql_hip_select_expr_dev(
                self._h, c_preds, k, c_nodes if n_nodes else None, n_nodes,
                ids[0].data_ptr() if ids[0] is not None and hi > lo else None, rows[0],
                ids[1].data_ptr() if ids[1] is not None and hi > lo else None, rows[1], hi - lo,
                out_a[m:].data_ptr() if out_a is not None and hi > lo else None,
                out_b[m:].data_ptr() if out_b is not None and hi > lo else None, ctypes.byref(kept), self._stream()))
            m += int(kept.value)
        return (out_a[:m] if out_a is not None else None, out_b[:m] if out_b is not None else None)

    #: programs per ``giql_hip_eval_expr_dev`` call
    EVAL_OUTS = 8

    def eval_exprs(self, trees, idx_a=None, idx_b=None, n=None, n_rows_a=0, n_rows_b=0):
        """The VALUE of every expression tree per candidate -- computed SELECT-list columns such as bedtools' -wo /
        -wao ``overlap_bp`` (``giql_hip_eval_expr_dev``): a list of ``(values, valid)`` device tensors, one per tree.

        ``trees`` are what :meth:`select` takes under ``("expr", tree)`` (with or without that wrapper), plus
        ``("if", cond, then, else)`` and ``("null",)``.  Candidates are the pairs ``(idx_a[i], idx_b[i])``; a missing
        id array means "the candidate index"; a NEGATIVE id is the NULL row of its side (every column of that side
        reads as NULL: the padded row of :meth:`left_pad`).  ``values`` is float64 where :func:`expr_can_float` says
        the tree can yield a float, else int64 (0 where NULL); ``valid`` is a uint8 tensor (0 = SQL NULL), or ``None``
        when the output holds no NULL.

        Any ``n`` is accepted: candidates go in slices of :attr:`SELECT_SLICE` as in :meth:`select`; more than
        :attr:`EVAL_OUTS` trees (or more than 256 nodes) go in several calls."""
        torch = _torch()
        if n is None:
            n = int((idx_a if idx_a is not None else idx_b).shape[0])
        n = int(n)
        for t in (idx_a, idx_b):
            if t is not None and (t.dtype != torch.int32 or not t.is_contiguous() or int(t.shape[0]) != n):
                raise ValueError("id arrays must be contiguous int32 tensors of n rows")
        trees = [t[1] if t[0] == "expr" else t for t in trees]
        flat = []
        for tree in trees:
            nodes, keep_alive = [], []
            self._flatten_expr(tree, nodes, keep_alive)
            if len(nodes) > 256:
                raise ValueError("at most 256 expression nodes per program")
            flat.append((nodes, keep_alive, expr_can_float(tree)))
        batches, cur, used = [], [], 0
        for k, (nodes, _ka, _fl) in enumerate(flat):
            if cur and (len(cur) == self.EVAL_OUTS or used + len(nodes) > 256):
                batches.append(cur)
                cur, used = [], 0
            cur.append(k)
            used += len(nodes)
        if cur:
            batches.append(cur)
        values = [torch.empty(n, dtype=torch.float64 if fl else torch.int64, device=self.device) for _n, _ka, fl in flat]
        valid = [torch.empty(n, dtype=torch.uint8, device=self.device) for _ in flat]
        n_null = [0] * len(flat)
        for batch in batches:
            nodes = [nd for k in batch for nd in flat[k][0]]
            c_nodes = (_lib.COperand * len(nodes))(*nodes)
            c_outs = (_lib.CExprOut * len(batch))()
            first = 0
            for j, k in enumerate(batch):
                c_outs[j].first, c_outs[j].count = first, len(flat[k][0])
                c_outs[j].type = _lib.T_F64 if flat[k][2] else _lib.T_I64
                first += len(flat[k][0])
            for lo in range(0, max(n, 1), self.SELECT_SLICE):
                hi = min(n, lo + self.SELECT_SLICE)
                ids, rows = [], []
                for t, n_rows in ((idx_a, int(n_rows_a)), (idx_b, int(n_rows_b))):
                    if t is not None:
                        t = t[lo:hi]
                    elif lo:    # (as in select: the candidate index stays global past the first slice)
                        t = torch.arange(lo, hi, dtype=torch.int32, device=self.device)
                        n_rows = n_rows or n
                    ids.append(t)
                    rows.append(n_rows)
                for j, k in enumerate(batch):
                    c_outs[j].data = values[k][lo:].data_ptr() if hi > lo else None
                    c_outs[j].valid = valid[k][lo:].data_ptr() if hi > lo else None
                nulls = (ctypes.c_int64 * len(batch))()
                _lib.check(self._L.giql_hip_eval_expr_dev(
                    self._h, c_nodes, len(nodes), c_outs, len(batch),
                    ids[0].data_ptr() if ids[0] is not None and hi > lo else None, rows[0],
                    ids[1].data_ptr() if ids[1] is not None and hi > lo else None, rows[1], hi - lo,
                    nulls, self._stream()))
                for j, k in enumerate(batch):
                    n_null[k] += int(nulls[j])
        return [(values[k], valid[k] if n_null[k] else None) for k in range(len(flat))]

    def range_set_any(self, chrom, start, end, sets, valid=(None, None, None)):
        """``interval <op> ANY(ranges)`` per row of one table, for up to 8 sets of up to 1024 literal ranges
        (``giql_hip_range_set_any_dev``): a list of ``(value, valid)`` uint8 device tensors, one pair per set --
        the predicate's three-valued result, ``valid`` 0 where it is SQL NULL -- ready to stand as a uint8 operand
        with its validity in :meth:`select`.

        ``chrom`` / ``start`` / ``end``: int32 device tensors of one length, the chromosome codes and the RAW
        coordinate columns; ``valid``: their uint8 validity tensors (``None`` = no NULLs).  A set is
        ``(op, chrom_codes, on_start, on_end)`` with ``op`` "intersects" / "contains" / "within" and three host
        sequences of one length: per range its chromosome code and the int64 bounds ``start`` and ``end`` are
        compared with (``start < on_start AND end > on_end`` for INTERSECTS, ``<=`` / ``>=`` for CONTAINS, ``>=`` /
        ``<=`` for WITHIN) -- the caller has moved the table's coordinate encoding onto them.  Any order, duplicates
        allowed."""
        import numpy as np

        torch = _torch()
        n = int(chrom.shape[0])
        cols = []
        for t, what in ((chrom, "chrom"), (start, "start"), (end, "end")):
            if t.dim() != 1 or int(t.shape[0]) != n:
                raise ValueError(f"{what} must be a 1-D tensor of {n} rows")
            cols.append(self._dev_ptr(t, what, torch.int32))
        valids = []
        for v, what in zip(valid, ("chrom", "start", "end")):
            if v is not None and (v.dtype not in (torch.uint8, torch.bool) or v.dim() != 1 or int(v.shape[0]) != n):
                raise ValueError(f"validity of {what} must be a uint8 tensor of {n} rows")
            valids.append(self._dev_ptr(v, f"validity of {what}"))
        if not 1 <= len(sets) <= _lib.RANGE_MAX_SETS:
            raise ValueError(f"between 1 and {_lib.RANGE_MAX_SETS} range sets per call, got {len(sets)}")
        c_sets = (_lib.CRangeSet * len(sets))()
        keep_alive, outs = [], []
        for j, (op, codes, on_start, on_end) in enumerate(sets):
            if op not in _lib.RANGE_OPS:
                raise ValueError(f"range set operator {op!r}")
            codes = np.ascontiguousarray(codes, dtype=np.int32)
            on_start = np.ascontiguousarray(on_start, dtype=np.int64)
            on_end = np.ascontiguousarray(on_end, dtype=np.int64)
            k = int(codes.shape[0])
            if codes.ndim != 1 or on_start.shape != codes.shape or on_end.shape != codes.shape:
                raise ValueError("a range set is three sequences of one length")
            if not 1 <= k <= _lib.RANGE_MAX_RANGES:
                raise ValueError(f"between 1 and {_lib.RANGE_MAX_RANGES} ranges per set, got {k}")
            value = torch.empty(n, dtype=torch.uint8, device=self.device)
            ok = torch.empty(n, dtype=torch.uint8, device=self.device)
            c_sets[j].op, c_sets[j].n_ranges = _lib.RANGE_OPS[op], k
            c_sets[j].chrom, c_sets[j].on_start, c_sets[j].on_end = codes.ctypes.data, on_start.ctypes.data, on_end.ctypes.data
            c_sets[j].out_value = value.data_ptr() if n else None
            c_sets[j].out_valid = ok.data_ptr() if n else None
            keep_alive.append((codes, on_start, on_end))
            outs.append((value, ok))
        _lib.check(self._L.giql_hip_range_set_any_dev(self._h, cols[0], cols[1], cols[2], valids[0], valids[1], valids[2],
                                                      n, c_sets, len(sets), self._stream()))
        return outs

    def mark(self, idx, n_rows: int):
        """``flags[idx] = 1`` over ``n_rows`` zero-initialised bytes (which left rows keep a pair)."""
        torch = _torch()
        flags = torch.zeros(int(n_rows), dtype=torch.uint8, device=self.device)
        n = int(idx.shape[0])
        if n:
            _lib.check(self._L.giql_hip_mark_dev(self._h, idx.data_ptr(), n, flags.data_ptr(), int(n_rows),
                                                 self._stream()))
        return flags

    # ------------------------------------------------------------- LEFT OUTER
    def left_pad(self, row_a, row_b, n_pairs: int, n_rows_a: int) -> int:
        """The unmatched-row pass of a LEFT OUTER join (``giql_hip_left_pad_dev``): behind the ``n_pairs`` pairs
        held at the front of ``row_a`` / ``row_b`` (int32 device tensors with room to spare; ``row_b`` may be
        ``None``), append ``(r, -1)`` for every ``r`` in ``[0, n_rows_a)`` that ``row_a[:n_pairs]`` does not hold,
        ascending.  Returns the new length.  Too little room raises ``GiqlHipError`` with ``GIQL_ERR_CAPACITY``
        and writes nothing; the length needed is then in :attr:`last_total`."""
        torch = _torch()
        cap = int(row_a.shape[0]) if row_b is None else min(int(row_a.shape[0]), int(row_b.shape[0]))
        if not 0 <= int(n_pairs) <= cap:
            raise ValueError(f"n_pairs = {n_pairs} outside [0, {cap}], the buffers' length")
        total = ctypes.c_int64(0)
        self.last_total = None
        rc = self._L.giql_hip_left_pad_dev(
            self._h, self._dev_ptr(row_a, "row_a", torch.int32), self._dev_ptr(row_b, "row_b", torch.int32),
            int(n_pairs), cap, int(n_rows_a), self._stream(), ctypes.byref(total))
        self.last_total = int(total.value)
        _lib.check(rc)
        return int(total.value)

    def left_join(self, a: DeviceSide, b: DeviceSide, n_chrom: int):
        """``a LEFT JOIN b ON a INTERSECTS b`` as row ids: the INNER join's pairs, then ``(r, -1)`` for every left
        row without a pair (ascending).  The pair buffers are allocated with room for ``a.n`` more entries that the
        join itself is never offered (:meth:`_join_into_buffers`), so the pad appends in place whatever the pair
        count turns out to be; the result is two views of them."""
        self._check_sides(a, b)
        row_a, row_b, n = self._join_into_buffers(a, b, n_chrom, extra_room=a.n)
        if min(int(row_a.shape[0]), int(row_b.shape[0])) < n + a.n:   # (joined group by group: exactly sized)
            return self.left_pad_pairs(row_a[:n], row_b[:n], a.n)
        total = self.left_pad(row_a, row_b, n, a.n)
        return row_a[:total], row_b[:total]

    def left_pad_pairs(self, ra, rb, n_rows_a: int):
        """:meth:`left_pad` for pairs that arrive in tensors of their own length (a join with residuals, CONTAINS,
        a within-distance join): they are copied once into buffers with room for ``n_rows_a`` more entries."""
        torch = _torch()
        n = int(ra.shape[0])
        row_a = torch.empty(n + int(n_rows_a), dtype=torch.int32, device=self.device)
        row_b = torch.empty(n + int(n_rows_a), dtype=torch.int32, device=self.device)
        row_a[:n] = ra
        row_b[:n] = rb
        total = self.left_pad(row_a, row_b, n, n_rows_a)
        return row_a[:total], row_b[:total]

    # --------------------------------------------------------------- checksum
    def pairs_checksum(self, row_a, row_b) -> int:
        torch = _torch()
        h = ctypes.c_uint64(0)
        n = min(int(row_a.shape[0]), int(row_b.shape[0]))
        _lib.check(self._L.giql_hip_pairs_checksum_dev(
            self._h, self._dev_ptr(row_a, "row_a", torch.int32), self._dev_ptr(row_b, "row_b", torch.int32), n,
            self._stream(), ctypes.byref(h)))
        return int(h.value)

    # ------------------------------------------ compact plan (multi-GPU exchange)
    def plan_export(self, q_rid, lo, cnt, s_rid, rid_add_a: int = 0, rid_add_b: int = 0):
        """Copy the last plan's compact form into caller tensors (``q_rid`` / ``lo`` / ``cnt`` of
        at least n_q int32 elements, ``s_rid`` of at least n_s), adding the two offsets to the A /
        B row ids; returns ``(query_is_a, n_q, n_s)``.  ``GIQL_ERR_STATE`` when the plan is not in
        the single-range form (exchange the pairs instead)."""
        qa, nq, ns = ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int64(0)
        qcap = min(int(q_rid.shape[0]), int(lo.shape[0]), int(cnt.shape[0]))
        scap = int(s_rid.shape[0])
        torch = _torch()
        _lib.check(self._L.giql_hip_inner_plan_export_dev(
            self._h, self._dev_ptr(q_rid, "q_rid", torch.int32), self._dev_ptr(lo, "lo", torch.int32),
            self._dev_ptr(cnt, "cnt", torch.int32), self._dev_ptr(s_rid, "s_rid", torch.int32), qcap, scap,
            int(rid_add_a), int(rid_add_b), ctypes.byref(qa), ctypes.byref(nq), ctypes.byref(ns), self._stream()))
        return bool(qa.value), int(nq.value), int(ns.value)

    def plan_sizes(self):
        """``(query_is_a, n_q, n_s)`` of the last plan's compact form without copying anything
        (the export call with empty buffers reports the sizes with ``GIQL_ERR_CAPACITY``)."""
        qa, nq, ns = ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int64(0)
        rc = self._L.giql_hip_inner_plan_export_dev(self._h, None, None, None, None, 0, 0, 0, 0, ctypes.byref(qa),
                                                    ctypes.byref(nq), ctypes.byref(ns), self._stream())
        if rc not in (_lib.GIQL_OK, _lib.GIQL_ERR_CAPACITY):
            _lib.check(rc)
        return bool(qa.value), int(nq.value), int(ns.value)

    def fill_from_plan(self, q_rid, lo, cnt, s_rid, row_q, row_s, n_pairs_expected: int = -1) -> int:
        """Expand a compact plan (this device's or another's) into ``row_q`` / ``row_s``; returns
        the pair count."""
        n = ctypes.c_int64(0)
        nq, ns = int(q_rid.shape[0]), int(s_rid.shape[0])
        cap = min(int(row_q.shape[0]), int(row_s.shape[0]))
        torch = _torch()
        i32 = torch.int32
        _lib.check(self._L.giql_hip_fill_from_plan_dev(
            self._h, self._dev_ptr(q_rid, "q_rid", i32), self._dev_ptr(lo, "lo", i32), self._dev_ptr(cnt, "cnt", i32),
            nq, self._dev_ptr(s_rid, "s_rid", i32), ns, self._dev_ptr(row_q, "row_q", i32),
            self._dev_ptr(row_s, "row_s", i32), cap, int(n_pairs_expected), self._stream(), ctypes.byref(n)))
        return int(n.value)

    # --------------------------------------------------------- host-buffer join
    def inner_join_host(self, a_cols, b_cols, n_chrom: int, offs_a=(0, 0), offs_b=(0, 0)):
        """``giql_hip_inner``: host (numpy int32) columns in, host index pairs out -- the
        PCIe-inclusive path (H2D of the six columns, join, D2H of the pairs into pinned memory).
        Returns two numpy arrays (copies; the library's buffers are released)."""
        import numpy as np

        def cside(cols, offs):
            c, s, e = (np.ascontiguousarray(x, np.int32) for x in cols)
            cs = _lib.CSide(c.ctypes.data, s.ctypes.data, e.ctypes.data, int(c.shape[0]), int(offs[0]), int(offs[1]))
            return cs, (c, s, e)

        ca, keep_a = cside(a_cols, offs_a)
        cb, keep_b = cside(b_cols, offs_b)
        n = ctypes.c_int64(0)
        pa, pb = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(self._L.giql_hip_inner(self._h, ctypes.byref(ca), ctypes.byref(cb), int(n_chrom),
                                          ctypes.byref(n), ctypes.byref(pa), ctypes.byref(pb)))
        try:
            m = int(n.value)
            ra = np.ctypeslib.as_array(ctypes.cast(pa, ctypes.POINTER(ctypes.c_int32)), shape=(max(m, 1),))[:m].copy()
            rb = np.ctypeslib.as_array(ctypes.cast(pb, ctypes.POINTER(ctypes.c_int32)), shape=(max(m, 1),))[:m].copy()
        finally:
            self._L.giql_hip_free_host(pa)
            self._L.giql_hip_free_host(pb)
        del keep_a, keep_b
        return ra, rb

    def inner_join_host_timed(self, a_cols, b_cols, n_chrom: int, inspect=None):
        """Wall time (ms) and pair count of one ``giql_hip_inner`` call; the pinned results are
        released without being copied (bench.py's t_e2e).  ``inspect(row_a, row_b)``: called with numpy views
        of the library-owned arrays before they are released (parity checks)."""
        import time

        import numpy as np

        def cside(cols):
            c, s, e = (np.ascontiguousarray(x, np.int32) for x in cols)
            return _lib.CSide(c.ctypes.data, s.ctypes.data, e.ctypes.data, int(c.shape[0]), 0, 0), (c, s, e)

        ca, keep_a = cside(a_cols)
        cb, keep_b = cside(b_cols)
        n = ctypes.c_int64(0)
        pa, pb = ctypes.c_void_p(), ctypes.c_void_p()
        t0 = time.perf_counter()
        rc = self._L.giql_hip_inner(self._h, ctypes.byref(ca), ctypes.byref(cb), int(n_chrom), ctypes.byref(n),
                                    ctypes.byref(pa), ctypes.byref(pb))
        ms = (time.perf_counter() - t0) * 1e3
        try:
            if rc == 0 and inspect is not None and n.value > 0:
                va = np.ctypeslib.as_array(ctypes.cast(pa, ctypes.POINTER(ctypes.c_int32)), shape=(int(n.value),))
                vb = np.ctypeslib.as_array(ctypes.cast(pb, ctypes.POINTER(ctypes.c_int32)), shape=(int(n.value),))
                inspect(va, vb)
                del va, vb
        finally:
            self._L.giql_hip_free_host(pa)
            self._L.giql_hip_free_host(pb)
        _lib.check(rc)
        del keep_a, keep_b
        return ms, int(n.value)

    # ---------------------------------------------------------------- copy probe
    def copy_probe(self, nbytes: int = 1600 << 20, reps: int = 5) -> float:
        """GB/s (read + written) of a 16-byte-per-lane copy of ``nbytes`` on this device."""
        torch = _torch()
        src = torch.empty(nbytes // 4, dtype=torch.int32, device=self.device)
        dst = torch.empty_like(src)
        src.fill_(1)
        g = ctypes.c_double(0.0)
        _lib.check(self._L.giql_hip_copy_probe_dev(self._h, src.data_ptr(), dst.data_ptr(), int(src.numel()) * 4,
                                                   int(reps), self._stream(), ctypes.byref(g)))
        return float(g.value)

    def stream_probe(self, nbytes: int = 1600 << 20, reps: int = 5, shapes=None) -> dict:
        """What this device reads / writes / copies per second (GB/s, every byte moved counted once), by access
        shape: ``{"read": best, "write": best, "copy": best, "memcpy_d2d": x, "shapes": {label: GB/s}}`` --
        16 B per lane with 1 / 4 / 8 accesses in flight, default and non-temporal cache policy, grids of
        ``n_cu x {4, 8, 16}`` blocks (``giql_hip_stream_probe_dev``).  The ceiling the kernels are held against."""
        torch = _torch()
        src = torch.empty(nbytes // 4, dtype=torch.int32, device=self.device)
        dst = torch.empty_like(src)
        src.fill_(1)
        dst.fill_(2)
        g = ctypes.c_double(0.0)

        def run(mode, in_flight, nt, per_cu):
            _lib.check(self._L.giql_hip_stream_probe_dev(
                self._h, src.data_ptr(), dst.data_ptr(), int(src.numel()) * 4, mode, in_flight, int(nt), per_cu,
                int(reps), self._stream(), ctypes.byref(g)))
            return float(g.value)

        if shapes is None:
            shapes = [(u, nt, per_cu) for u in (1, 4, 8) for nt in (0, 1) for per_cu in (4, 8, 16)]
        out = {"shapes": {}}
        for name, mode in (("read", 0), ("write", 1), ("copy", 2)):
            best = 0.0
            for u, nt, per_cu in shapes:
                v = run(mode, u, nt, per_cu)
                out["shapes"][f"{name}/x{u}/{'nt' if nt else 'dflt'}/{per_cu}perCU"] = round(v, 1)
                best = max(best, v)
            out[name] = round(best, 1)
        out["memcpy_d2d"] = round(run(3, 1, 0, 8), 1)
        return out

    @staticmethod
    def host_pool_trim(keep_bytes: int = 0) -> int:
        """Return idle page-locked output buffers of the host-buffer entry points to the OS; bytes released."""
        freed = ctypes.c_int64(0)
        _lib.check(_lib.load().giql_hip_host_pool_trim(int(keep_bytes), ctypes.byref(freed)))
        return int(freed.value)
