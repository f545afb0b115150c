"""``execute(plan, tables)`` -- run a ``dialect="hip"`` plan on the GPU.

The reference hands its SQL string to an engine (``conn.execute(sql)``,
``docs/transpilation/execution.rst:4-30``); this is the hip target's counterpart:
plan string + Arrow tables in, Arrow table out.  Host work here is boundary
plumbing only -- dictionary-encoding ``chrom`` with a dictionary SHARED by both
sides (the reference compares VARCHAR values), int32 range
checks, the H2D copy, and the final ``take`` of the projected columns by the
returned row indices.  The join itself runs in ``libgiql_hip.so``.
"""

from __future__ import annotations

import os
import re
import threading

import numpy as np

from ._lib import GIQL_ERR_CAPACITY, GiqlHipError
from .engine import ENCODING_OFFSETS, DeviceSide, HipEngine, InvertedRows
from .plan import JoinPlan, PlanSide, Projection, is_plan_string
from .shape import operand_sides
from .transpile import build_plan

_ENGINES: dict[int, HipEngine] = {}


def default_engine(device: int = 0) -> HipEngine:
    if device not in _ENGINES:
        _ENGINES[device] = HipEngine(device)
    return _ENGINES[device]


def _column(table, name: str):
    """Fetch a column from a pyarrow.Table / dict / pandas.DataFrame as an array."""
    try:
        import pyarrow as pa
    except ImportError:  # pragma: no cover
        pa = None
    if pa is not None and isinstance(table, pa.Table):
        if name not in table.column_names:
            raise ValueError(f"column {name!r} not found (have {table.column_names})")
        return table.column(name)
    try:
        return table[name]
    except (KeyError, IndexError) as exc:
        raise ValueError(f"column {name!r} not found") from exc


def _n_rows(table) -> int:
    if hasattr(table, "num_rows"):
        return int(table.num_rows)
    first = next(iter(table.values())) if isinstance(table, dict) else table.iloc[:, 0]
    return len(first)


def _to_numpy(col, what: str) -> np.ndarray:
    try:
        import pyarrow as pa

        if isinstance(col, (pa.ChunkedArray, pa.Array)):
            if col.null_count:
                # SQL NULL never matches; the C ABI wants all-valid buffers
                raise ValueError(f"{what} contains NULLs: not supported by dialect='hip'")
            return col.to_numpy(zero_copy_only=False) if isinstance(col, pa.Array) else col.combine_chunks().to_numpy(zero_copy_only=False)
    except ImportError:  # pragma: no cover
        pass
    return np.asarray(col)


def _to_numpy_obj(col) -> np.ndarray:
    """A column as a numpy object array with None for NULL (strings / strands)."""
    try:
        import pyarrow as pa

        if isinstance(col, (pa.ChunkedArray, pa.Array)):
            return np.array(col.to_pylist(), dtype=object)
    except ImportError:  # pragma: no cover
        pass
    return np.asarray(col, dtype=object)


def _int32_column(col, what: str) -> np.ndarray:
    x = _to_numpy(col, what)
    if x.dtype.kind not in "iu":
        raise ValueError(f"{what} must be an integer column, got {x.dtype}")
    if x.size and (x.min() < -(2**31) or x.max() > 2**31 - 1):
        raise ValueError(f"{what} does not fit int32 (the hip path joins int32 coordinates)")
    return np.ascontiguousarray(x, dtype=np.int32)


# ---------------------------------------------------------------------------------------------------------
# What may be kept between calls.  A device copy / a dictionary encoding of a column is only valid while the
# column's MEMORY is what it was, and an Arrow array does not own that question: ``pa.array(numpy_int32)`` and
# ``pa.Table.from_pandas(df)`` alias the numpy memory zero-copy (an in-place ``x[0] = 99`` shows through the
# Arrow array), and Arrow's own pool buffers report ``is_mutable`` as well.  So nothing is kept implicitly
# unless every buffer of the column is immutable (memory-mapped / IPC-read files, read-only numpy arrays);
# everything else is kept only for tables the caller has PINNED -- ``giql_amd.pin(table)``: an explicit promise
# that the table's memory will not be written while the pin lives (VERDICT r03 weak #2 / ADVICE r03).
# ---------------------------------------------------------------------------------------------------------
_CODES_CACHE: "OrderedDict" = None      # (buffer addresses, offset, length, type, nulls_as) -> (the column, its codes, idents)
_CODES_CACHE_SLOTS = int(os.environ.get("GIQL_HIP_CODES_CACHE_SLOTS", "6"))   # 0: nothing is kept between calls
_CODES_CACHE_MIN_ROWS = 1_000_000
_CODES_LOCK = threading.Lock()
_PINNED: dict = {}       # identity of a pinned column chunk -> number of live pins holding it


def _chunk_ident(c) -> tuple:
    """Identity of one Arrow array by its memory: buffer addresses, offset, length (a dictionary array's values
    live in buffers of their own: part of its identity)."""
    own = (tuple(b.address if b is not None else 0 for b in c.buffers()), c.offset, len(c))
    return own + _chunk_ident(c.dictionary) if hasattr(c, "dictionary") else own


def _col_idents(col) -> tuple:
    return tuple(_chunk_ident(c) for c in (col.chunks if hasattr(col, "chunks") else [col]))


def _frozen(col) -> bool:
    """Nothing can write this column's memory behind Arrow's back: every chunk is pinned by the caller, or every
    buffer it has is immutable."""
    def immutable(c):
        bufs = list(c.buffers()) + (list(c.dictionary.buffers()) if hasattr(c, "dictionary") else [])
        return all(b is None or not b.is_mutable for b in bufs)

    chunks = col.chunks if hasattr(col, "chunks") else [col]
    with _CODES_LOCK:
        pinned = all(_chunk_ident(c) in _PINNED for c in chunks)
    return pinned or all(immutable(c) for c in chunks)


class PinnedTable:
    """``giql_amd.pin(table)``: the caller's promise that the table's memory stays as it is while the pin lives.

    ``execute()`` then keeps what it derives from the table between calls -- the device copy of the genomic
    columns (1.3 GB over PCIe for a 100M-row table: 0.11-0.16 s of a 0.35 s join), the dictionary codes of its
    string columns (~1 s of hashing at that size) -- and, for ``index=True``, a sorted index in HBM
    (``giql_hip_index_create_dev``).  Pass the handle (or the table itself) in ``tables=``; ``unpin()`` /
    ``with pin(t) as p:`` / garbage collection ends the promise and drops everything derived.  After changing
    the table in place: ``refresh()``.  The reference's counterpart is the engine's own table + ``CREATE INDEX
    ... (chrom, start, "end")`` (``docs/transpilation/performance.rst:111-130``)."""

    def __init__(self, table, index: bool = False):
        import pyarrow as pa

        if isinstance(table, PinnedTable):
            table = table.table
        if not isinstance(table, pa.Table):
            table = pa.table(table) if isinstance(table, dict) else pa.Table.from_pandas(table)
        self.table = table
        self.index = bool(index)
        self._indexes: dict = {}    # (device, chrom / start / end columns, encoding) -> (DeviceIndex | None, dictionary)
        self._idents = [i for name in table.column_names for i in _col_idents(table.column(name))]
        self._live = True
        with _CODES_LOCK:
            for i in self._idents:
                _PINNED[i] = _PINNED.get(i, 0) + 1

    # (an Arrow table's reading interface, so that a handle can stand wherever the table stood)
    @property
    def num_rows(self):
        return self.table.num_rows

    @property
    def column_names(self):
        return self.table.column_names

    def column(self, name):
        return self.table.column(name)

    def __getitem__(self, name):
        return self.table[name]

    def refresh(self) -> None:
        """The table was changed in place: drop what was derived from it (the next call derives it again)."""
        _drop_derived(set(self._idents))
        self._drop_indexes()

    def _drop_indexes(self) -> None:
        for idx, _d in self._indexes.values():
            if idx is not None:
                idx.close()
        self._indexes.clear()

    def index_info(self) -> list:
        """``[{"device", "rows", "hbm_bytes", "form"}]`` of the indexes built so far (one per device / column set)."""
        return [{"device": k[0], "rows": i.n, "hbm_bytes": i.nbytes, "form": "general" if i.general else "fixed_length"}
                for k, (i, _d) in self._indexes.items() if i is not None]

    def unpin(self) -> None:
        if not self._live:
            return
        self._live = False
        gone = set()
        with _CODES_LOCK:
            for i in self._idents:
                n = _PINNED.get(i, 0) - 1
                if n <= 0:
                    _PINNED.pop(i, None)
                    gone.add(i)
                else:
                    _PINNED[i] = n
        _drop_derived(gone)
        self._drop_indexes()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.unpin()

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.unpin()
        except Exception:
            pass


def pin(table, index: bool = False) -> PinnedTable:
    """See :class:`PinnedTable`.  ``index=True``: INNER, SEMI, ANTI and count_overlaps joins against this table go
    through a table index in HBM, built on first use (``giql_hip_index_create_dev``: the table's span pass and global
    sort passes are then not repeated per query; SEMI / ANTI / count_overlaps with the table on the RIGHT sort
    neither side) -- the counterpart of ``CREATE INDEX ... (chrom, start, "end")``.  NEAREST (k = 1, unstranded) with
    the table as its target reads the same index for the index forms ``_INDEXED_NEAREST_FORMS`` switches on."""
    return PinnedTable(table, index=index)


def _unwrap(table):
    return table.table if isinstance(table, PinnedTable) else table


def _drop_derived(idents: set) -> None:
    """Forget every cached encoding / device copy that was derived from one of these column chunks."""
    if not idents:
        return
    with _CODES_LOCK:
        for cache in (_CODES_CACHE, _SIDES_CACHE):
            if cache:
                for key in [k for k, v in cache.items() if idents & v[2]]:
                    del cache[key]


def clear_caches(host_pool: bool = True) -> dict:
    """Drop everything ``execute()`` keeps between calls: dictionary codes, device copies of tables (HBM), and --
    ``host_pool`` -- the idle page-locked output buffers of the C library's host-buffer entry points.  Pins stay
    (their tables are simply derived again).  Returns what was held: ``{"codes": entries, "sides": entries,
    "hbm_bytes": n, "host_pool_bytes": n}``."""
    held = cache_info()
    with _CODES_LOCK:
        if _CODES_CACHE:
            _CODES_CACHE.clear()
        if _SIDES_CACHE:
            _SIDES_CACHE.clear()
    held["host_pool_bytes"] = HipEngine.host_pool_trim(0) if host_pool else 0
    return held


def cache_info() -> dict:
    """What the caches hold now: entries, and the HBM bytes of the device copies (12 B per cached row)."""
    with _CODES_LOCK:
        sides = list(_SIDES_CACHE.values()) if _SIDES_CACHE else []
        return {"codes": len(_CODES_CACHE) if _CODES_CACHE else 0, "sides": len(sides),
                "hbm_bytes": sum(12 * v[1].n for v in sides), "pinned_chunks": len(_PINNED)}


def _cached_codes(col, nulls_as, compute):
    """The codes of a long column are kept for the next query over the same memory (hashing 110M strings is ~1 s
    of a ~1.7 s INNER join of BASELINE size) -- when that memory cannot change (``_frozen``: pinned by the caller,
    or immutable buffers).  The entry holds the column, so its buffers cannot be freed and their addresses reused
    while it is cached; a handful of slots, oldest out."""
    global _CODES_CACHE
    cols = col if isinstance(col, tuple) else (col,)          # (a pair: the shared encoding of two columns)
    if (sum(len(c) for c in cols) < _CODES_CACHE_MIN_ROWS or _CODES_CACHE_SLOTS <= 0
            or not all(_frozen(c) for c in cols)):
        return compute()
    if _CODES_CACHE is None:
        from collections import OrderedDict

        _CODES_CACHE = OrderedDict()
    idents = frozenset(i for one in cols for i in _col_idents(one))
    key = (tuple((_col_idents(one), str(one.type)) for one in cols), nulls_as)
    with _CODES_LOCK:
        hit = _CODES_CACHE.get(key)
        if hit is not None:
            _CODES_CACHE.move_to_end(key)
            return hit[1]
    value = compute()
    with _CODES_LOCK:
        _CODES_CACHE[key] = (col, value, idents)
        while len(_CODES_CACHE) > _CODES_CACHE_SLOTS:
            _CODES_CACHE.popitem(last=False)
    return value


def _arrow_codes(col, what: str, nulls_as=None):
    """An Arrow string / dictionary column as ``(int32 codes, dictionary values)`` through Arrow's own hash
    (``pyarrow.compute.dictionary_encode``: ~0.8 s per 100M rows where a Python-level pass takes minutes), or
    None when the column is not one.  NULLs are refused as everywhere unless ``nulls_as``
    names the value they are encoded as (the caller carries the validity beside)."""
    try:
        import pyarrow as pa
        import pyarrow.compute as pc
    except ImportError:  # pragma: no cover
        return None
    if not isinstance(col, (pa.Array, pa.ChunkedArray)):
        return None
    t = col.type
    value_type = t.value_type if pa.types.is_dictionary(t) else t
    if not (pa.types.is_string(value_type) or pa.types.is_large_string(value_type)):
        return None

    def compute():
        c = col
        if isinstance(c, pa.ChunkedArray):
            if c.num_chunks == 1:
                c = c.chunk(0)
            elif pa.types.is_dictionary(t):
                c = c.unify_dictionaries().combine_chunks()
            else:
                c = c.combine_chunks()
        ty = c.type
        if c.null_count or (pa.types.is_dictionary(ty) and c.dictionary.null_count):
            if nulls_as is None:
                raise ValueError(f"{what} contains NULLs: not supported by dialect='hip'")
            c = (c.dictionary_decode() if pa.types.is_dictionary(ty) else c).fill_null(nulls_as)
            ty = c.type
        d = c if pa.types.is_dictionary(ty) else pc.dictionary_encode(c)
        return d.indices.to_numpy(zero_copy_only=False), d.dictionary.to_pylist()

    return _cached_codes(col, nulls_as, compute)


def _sorted_union_codes(parts):
    """``[(codes, values)]`` -> (codes re-expressed in ONE sorted dictionary, that dictionary).  Sorted like
    ``numpy.unique`` sorts strings, so an id order is a chromosome-name order (MERGE's ORDER BY relies on it)."""
    dictionary = sorted(set().union(*[set(v) for _c, v in parts]))
    pos = {v: i for i, v in enumerate(dictionary)}
    out = []
    for codes, values in parts:
        lut = np.fromiter((pos[v] for v in values), dtype=np.int32, count=len(values))
        out.append(np.ascontiguousarray(lut[codes]) if len(values) else np.zeros(0, np.int32))
    return out, dictionary


def _refuse_null_chroms(values: np.ndarray) -> None:
    """SQL NULL never matches (and the reference never joins NULL chroms): every element is checked, not
    the first -- a later None would otherwise become the string 'None' in a dictionary and NULL-chrom rows
    of the two sides would join each other."""
    if values.size:
        null = np.fromiter((v is None or (isinstance(v, float) and v != v) for v in values.astype(object, copy=False)),
                           dtype=bool, count=values.size)
        if null.any():
            raise ValueError("chrom contains NULLs: not supported by dialect='hip'")


def encode_chroms(col_a, col_b):
    """Shared dictionary encoding of both chrom columns -> (ids_a, ids_b, dictionary)."""
    fast = [_arrow_codes(col_a, "left chrom column"), _arrow_codes(col_b, "right chrom column")]
    if fast[0] is not None and fast[1] is not None:
        def shared():
            (ia, ib), dictionary = _sorted_union_codes(fast)
            ia.setflags(write=False)      # (shared by every later query over these tables)
            ib.setflags(write=False)
            return ia, ib, dictionary

        ia, ib, dictionary = _cached_codes((col_a, col_b), "pair", shared)
        return ia, ib, list(dictionary)
    a = _to_numpy(col_a, "left chrom column")
    b = _to_numpy(col_b, "right chrom column")
    if a.dtype.kind in "iu" and b.dtype.kind in "iu":
        ia, ib = _int32_column(a, "left chrom"), _int32_column(b, "right chrom")
        if (ia.size and ia.min() < 0) or (ib.size and ib.min() < 0):
            raise ValueError("integer chrom ids must be non-negative")
        n = int(max(ia.max() if ia.size else -1, ib.max() if ib.size else -1)) + 1
        if n > 4096 and n > 4 * (ia.size + ib.size):
            # sparse ids (one large id would size every per-chromosome array by it): remap to dense codes
            dictionary, inverse = np.unique(np.concatenate([ia, ib]), return_inverse=True)
            inverse = inverse.astype(np.int32)
            return (np.ascontiguousarray(inverse[: ia.size]), np.ascontiguousarray(inverse[ia.size:]),
                    dictionary.tolist())
        return ia, ib, list(range(n))
    both = np.concatenate([a.astype(object), b.astype(object)])
    _refuse_null_chroms(both)
    dictionary, inverse = np.unique(both.astype(str), return_inverse=True)
    inverse = inverse.astype(np.int32)
    return (np.ascontiguousarray(inverse[: a.size]), np.ascontiguousarray(inverse[a.size:]),
            dictionary.tolist())


_SIDES_CACHE = None      # (start / end buffers, the chrom-id array, device, encoding) -> (what keeps those alive, DeviceSide, idents)
_SIDES_CACHE_SLOTS = int(os.environ.get("GIQL_HIP_SIDES_CACHE_SLOTS", "4"))   # 0: every call uploads its tables


def _device_side(table, side: PlanSide, chrom_ids: np.ndarray, engine: HipEngine) -> DeviceSide:
    """The (chrom id, start, end) columns of a table on the device.  A long table whose memory cannot change
    (``_frozen``: pinned with ``giql_amd.pin``, or immutable Arrow buffers) is not uploaded again (1.3 GB over PCIe
    from pageable memory is 0.11-0.16 s of a 0.35 s INNER join of BASELINE size): the entry holds the columns and
    the id array, so neither their buffers nor the array's ``id`` can be reused while it lives.  Up to
    ``GIQL_HIP_SIDES_CACHE_SLOTS`` (4) tables, 12 bytes of HBM per row each; ``clear_caches()`` drops them."""
    global _SIDES_CACHE
    scol, ecol = _column(table, side.start_col), _column(table, side.end_col)
    key = None
    try:
        import pyarrow as pa

        if (_SIDES_CACHE_SLOTS > 0 and len(chrom_ids) >= _CODES_CACHE_MIN_ROWS and not chrom_ids.flags.writeable
                and all(isinstance(c, (pa.Array, pa.ChunkedArray)) for c in (scol, ecol))
                and _frozen(scol) and _frozen(ecol)):
            key = (_col_idents(scol), _col_idents(ecol), id(chrom_ids), str(engine.device), side.encoding)
    except ImportError:  # pragma: no cover
        pass
    if key is not None:
        if _SIDES_CACHE is None:
            from collections import OrderedDict

            _SIDES_CACHE = OrderedDict()
        with _CODES_LOCK:
            hit = _SIDES_CACHE.get(key)
            if hit is not None:
                _SIDES_CACHE.move_to_end(key)
                return hit[1]
    start = _int32_column(scol, f"{side.table}.{side.start_col}")
    end = _int32_column(ecol, f"{side.table}.{side.end_col}")
    dev = DeviceSide.from_numpy(chrom_ids, start, end, side.encoding, device=engine.device)
    if key is not None:
        with _CODES_LOCK:
            _SIDES_CACHE[key] = ((scol, ecol, chrom_ids), dev, frozenset(key[0] + key[1]))
            while len(_SIDES_CACHE) > _SIDES_CACHE_SLOTS:
                _SIDES_CACHE.popitem(last=False)
    return dev


def _take(table, name: str, idx: np.ndarray, pad_null: bool = False):
    """``pad_null`` (the right side of a LEFT plan): a row id of -1 yields NULL."""
    col = _column(table, name)
    pad = (idx < 0) if pad_null else None
    try:
        import pyarrow as pa

        if isinstance(col, (pa.ChunkedArray, pa.Array)):
            return col.take(pa.array(idx, type=pa.int64(), mask=pad))
    except ImportError:  # pragma: no cover
        pass
    if pad is None:
        return np.asarray(col)[idx]
    vals = np.asarray(col)
    if not vals.shape[0]:       # (an empty right table: every row is padded)
        vals = np.zeros(1, vals.dtype)
    return np.ma.masked_array(vals[np.where(pad, 0, idx)], mask=pad)


class _Residuals:
    """Bind a plan's residual predicates to device columns for ``HipEngine.select``.

    Numeric columns are uploaded as int32 / int64 / float32 / float64 / uint8; a
    string comparison (column vs column or column vs literal) is dictionary-encoded
    with one SORTED dictionary shared by both operands, so ``=`` / ``<`` on the int32
    codes is the comparison on the strings (binary collation).  Validity bitmaps
    travel as byte columns: a NULL operand makes the predicate not true.
    """

    def __init__(self, plan: JoinPlan, lt, rt, eng: HipEngine, dev_sides=None):
        self.plan, self.tables, self.eng = plan, {"l": lt, "r": rt}, eng  # rt is None for CLUSTER / MERGE
        self._cache: dict = {}
        # the genomic columns are on the device already (raw values, as SQL sees them): a condition over a.start /
        # b.end -- the overlap-fraction recipes -- reads those tensors instead of uploading the columns again
        for key, dev in (dev_sides or {}).items():
            ps = plan.left if key == "l" else plan.right
            if dev is not None and ps is not None and ps.start_col != ps.end_col:
                self._cache[(key, ps.start_col)] = (dev.start, None)
                self._cache[(key, ps.end_col)] = (dev.end, None)

    @staticmethod
    def sides(clause) -> set:
        """The tables a clause (a list of OR-ed residuals) reads."""
        return set().union(*[operand_sides(o) for res in clause for o in (res.lhs, res.rhs)])

    @staticmethod
    def clauses(residuals) -> list:
        """Residuals are AND-ed; neighbours sharing a non-zero group form one OR clause."""
        out: list = []
        for r in residuals:
            if out and r.group and out[-1][-1].group == r.group:
                out[-1].append(r)
            else:
                out.append([r])
        return out

    def _arrow(self, side: str, column: str):
        import pyarrow as pa

        col = _column(self.tables[side], column)
        if isinstance(col, pa.ChunkedArray):
            col = col.combine_chunks() if col.num_chunks != 1 else col.chunk(0)
        if not isinstance(col, pa.Array):
            col = pa.array(np.asarray(col))
        if pa.types.is_dictionary(col.type):
            col = col.dictionary_decode()
        return col

    def _valid(self, col):
        import torch

        if not col.null_count:
            return None
        return torch.from_numpy(np.ascontiguousarray(col.is_valid().to_numpy(zero_copy_only=False).astype(np.uint8))
                                ).to(self.eng.device)

    def _numeric(self, side: str, column: str):
        import pyarrow as pa
        import torch

        key = (side, column)
        if key in self._cache:
            return self._cache[key]
        col = self._arrow(side, column)
        t = col.type
        if pa.types.is_boolean(t):
            vals = col.fill_null(False).to_numpy(zero_copy_only=False).astype(np.uint8)
        elif pa.types.is_integer(t):
            vals = col.fill_null(0).to_numpy(zero_copy_only=False)
            if vals.dtype == np.uint64:
                if vals.size and vals.max() > np.iinfo(np.int64).max:
                    raise ValueError(f"column {column!r}: uint64 values beyond int64 are not supported in a predicate")
                vals = vals.astype(np.int64)
            elif vals.dtype.itemsize < 4 or vals.dtype == np.int32:
                vals = vals.astype(np.int32)
            else:
                vals = vals.astype(np.int64)
        elif pa.types.is_floating(t):
            vals = col.fill_null(0).to_numpy(zero_copy_only=False)
            vals = vals.astype(np.float64 if vals.dtype == np.float64 else np.float32)
        else:
            return None
        out = (torch.from_numpy(np.ascontiguousarray(vals)).to(self.eng.device), self._valid(col))
        self._cache[key] = out
        return out

    def _is_string_column(self, side: str, column: str) -> bool:
        import pyarrow as pa

        t = self._arrow(side, column).type
        return pa.types.is_string(t) or pa.types.is_large_string(t)

    def _is_string(self, o) -> bool:
        if o.kind == "str":
            return True
        if o.kind in ("l", "r"):
            return self._is_string_column(o.kind, o.value)
        return False

    def pred(self, res):
        """``(lhs_spec, op, rhs_spec)`` for :meth:`HipEngine.select`; left = side "a"."""
        import torch

        ops = (res.lhs, res.rhs)
        eside = {"l": "a", "r": "b"}
        if res.op == "istrue":                # a whole boolean condition as one program
            return self._spec(res.lhs), "istrue", ("lit", 0), res.group
        if res.op in ("isnull", "notnull"):   # reads the validity of lhs only, whatever the column's type
            if res.lhs.kind == "expr":        # (a.score + 1) IS NULL: the kernel tells the expression's own NULL
                return self._spec(res.lhs), res.op, ("lit", 0), res.group
            col = self._arrow(res.lhs.kind, res.lhs.value)
            data = torch.zeros(len(col), dtype=torch.uint8, device=self.eng.device)
            return (eside[res.lhs.kind], data, self._valid(col)), res.op, ("lit", 0), res.group
        if any(o.kind == "expr" for o in ops) and not any(self._is_string(o) for o in ops):
            return self._spec(ops[0]), res.op, self._spec(ops[1]), res.group
        if any(self._is_string(o) for o in ops):
            specs = self._string_pair(ops, res.op)
            return specs[0], res.op, specs[1], res.group
        return self._spec(ops[0]), res.op, self._spec(ops[1]), res.group

    def _string_pair(self, ops, op):
        """Two string operands (columns / literals) of ONE comparison as int32 codes of one sorted dictionary
        shared by both: ``=`` / ``<`` on the codes is ``=`` / ``<`` on the strings (binary collation)."""
        import torch

        from .plan import Operand

        eside = {"l": "a", "r": "b"}
        ops = [o if isinstance(o, Operand) else Operand(o[0], o[1]) for o in ops]
        if not all(self._is_string(o) for o in ops):
            raise ValueError(f"cannot compare a string with a number in {ops[0].value!r} {op} {ops[1].value!r}")
        parts = []
        for o in ops:
            if o.kind == "str":
                parts.append((np.zeros(1, np.int32), [o.value]))
            else:   # (the raw column first: its buffers are the cache's key; _arrow() may build a new array)
                coded = _arrow_codes(_column(self.tables[o.kind], o.value), o.value, nulls_as="")
                parts.append(coded if coded is not None else _arrow_codes(self._arrow(o.kind, o.value), o.value, nulls_as=""))
        coded, _dictionary = _sorted_union_codes(parts)
        specs = []
        for o, codes in zip(ops, coded):
            if o.kind == "str":
                specs.append(("lit", int(codes[0])))
            else:
                col = self._arrow(o.kind, o.value)
                specs.append((eside[o.kind], torch.from_numpy(np.ascontiguousarray(codes, dtype=np.int32)).to(self.eng.device),
                              self._valid(col)))
        return specs

    def _spec(self, o, where: str = "predicate"):
        """An operand as :meth:`HipEngine.select` takes it: a column, a literal, or ``("expr", tree)`` -- arithmetic,
        or (round 4) a whole boolean condition: comparisons, IS [NOT] NULL, AND / OR / NOT
        (``giql_hip_select_expr_dev``); a computed column's searched CASE comes out as ``("if", cond, then, else)`` /
        ``("null",)`` for :meth:`HipEngine.eval_exprs`.  ``where`` names the operand's place in an error."""
        import torch

        eside = {"l": "a", "r": "b"}

        def leaf(kind, value):
            if kind in ("int", "float"):
                return ("lit", value)
            nv = self._numeric(kind, value)
            if nv is None:
                raise ValueError(f"column {value!r}: type {self._arrow(kind, value).type} is not supported "
                                 f"in a dialect='hip' {where}" + (" expression" if o.kind == "expr" else ""))
            return (eside[kind], nv[0], nv[1])

        def is_str(t):
            return t[0] == "str" or (t[0] in ("l", "r") and self._is_string_column(t[0], t[1]))

        def tree(t):
            if t[0] != "fn":
                return leaf(t[0], t[1])
            op, kids = t[1], t[2]
            if op in ("isnull", "notnull") and kids[0][0] in ("l", "r"):
                # the validity of a column, whatever its type
                col = self._arrow(kids[0][0], kids[0][1])
                key = (kids[0][0], kids[0][1], "valid")
                if key not in self._cache:
                    self._cache[key] = (torch.zeros(len(col), dtype=torch.uint8, device=self.eng.device), self._valid(col))
                data, valid = self._cache[key]
                return (op, (eside[kids[0][0]], data, valid))
            if op in ("=", "!=", "<", "<=", ">", ">=") and any(is_str(c) for c in kids):
                if any(c[0] == "fn" for c in kids):
                    raise ValueError("cannot compare a string with an arithmetic expression")
                return (op, *self._string_pair(kids, op))
            return (op, *[tree(c) for c in kids])

        return ("expr", tree(o.value)) if o.kind == "expr" else leaf(o.kind, o.value)

    def preds(self, clauses):
        """The predicates of a list of clauses (or of plain residuals), in order."""
        return [self.pred(r) for c in clauses for r in (c if isinstance(c, list) else [c])]


def _subset(eng: HipEngine, side: DeviceSide, ids):
    """The rows ``ids`` of a device side (a prefilter's survivors)."""
    if ids is None:
        return side
    c, s, e = eng.take([side.chrom, side.start, side.end], ids)
    return DeviceSide(c, s, e, side.start_off, side.end_off)


def _spatial_join(plan: JoinPlan, a: DeviceSide, b: DeviceSide, n_chrom: int, eng: HipEngine):
    """The pairs ``(row_left, row_right)`` of an INNER plan's spatial predicate: INTERSECTS, or CONTAINS / WITHIN
    (src/giql/expanders/intersects.py:155-166) through the one containment path, ``contain_join(outer, inner)`` --
    WITHIN with the sides exchanged and the result columns exchanged back."""
    if plan.predicate == "within_distance":
        # DISTANCE(left, right) <= max_distance: the INNER join over the widened left side (HipEngine.window_join)
        if plan.max_distance < 0:       # written "< 0": a distance is never negative
            import torch

            z = torch.empty(0, dtype=torch.int32, device=eng.device)
            return z, z.clone()
        try:
            return eng.window_join(a, b, n_chrom, plan.max_distance)
        except InvertedRows as exc:
            raise _inverted_rows_error(plan, exc) from exc
    if plan.predicate == "contains":
        return eng.contain_join(a, b, n_chrom)
    if plan.predicate == "within":
        rb, ra = eng.contain_join(b, a, n_chrom)
        return ra, rb
    return eng.inner_join(a, b, n_chrom)


# SEMI / ANTI ("exists") and count_overlaps ("count") over CONTAINS / WITHIN / DISTANCE <= N, per form: True = execute()
# calls HipEngine.semi_anti_pred / count_pred, False = it composes what existed before them (the pair join, then mark
# + select, or a bincount of the left ids).  A form is on only where the new call's median lay below the
# composition's whole spread at BOTH sizes of tools/row_predicates_timing.py (the rule of _INDEXED_NEAREST_FORMS);
# a form that is off stays reachable through the engine method.  Measured (profiles/row_predicates_timing.json.log;
# new ms against composed [min, max] ms at 1M x 10M, then at 100M x 10M; DESIGN.md "Row predicates" has the table):
#   exists / contains          0.494 vs [0.622, 0.735]   6.74 vs [5.20, 5.47]    -> off (loses where no pair exists)
#   exists / within            0.456 vs [0.827, 0.850]   7.07 vs [7.69, 7.91]    -> on
#   exists / within_distance   0.461 vs [0.721, 0.733]   7.08 vs [23.3, 23.7]    -> on
#   count  / contains          0.458 vs [0.746, 0.878]   5.43 vs [4.81, 4.92]    -> off (loses where no pair exists)
#   count  / within            0.763 vs [0.769, 0.783]   8.09 vs [18.2, 18.3]    -> on (the small size by 0.006 ms)
#   count  / within_distance   0.595 vs [1.227, 1.242]   7.48 vs [67.2, 67.8]    -> on
_ROW_PREDICATE_FORMS = {
    ("exists", "contains"): False, ("exists", "within"): True, ("exists", "within_distance"): True,
    ("count", "contains"): False, ("count", "within"): True, ("count", "within_distance"): True,
}


def _inverted_rows_error(plan: JoinPlan, exc: InvertedRows) -> ValueError:
    bad = " and ".join(repr((plan.left if s == "a" else plan.right).table) for s in exc.sides)
    return ValueError(f"DISTANCE needs start <= end on every row: table {bad} has a row with start > end")


def _row_pred_matched(plan: JoinPlan, a: DeviceSide, b: DeviceSide, n_chrom: int, eng: HipEngine, anti: bool):
    """Ascending ids of the ``a`` rows with / without a ``b`` row under the plan's CONTAINS / WITHIN / DISTANCE
    predicate: the engine's per-row call, or the pair join reduced by mark + select where that measured no slower
    (``_ROW_PREDICATE_FORMS``)."""
    if _ROW_PREDICATE_FORMS[("exists", plan.predicate)]:
        try:
            return eng.semi_anti_pred(a, b, n_chrom, plan.predicate, anti, plan.max_distance)
        except InvertedRows as exc:
            raise _inverted_rows_error(plan, exc) from exc
    ra, _rb = _spatial_join(plan, a, b, n_chrom, eng)
    flags = eng.mark(ra.contiguous(), a.n)
    return eng.select([(("a", flags), "=", ("lit", 0 if anti else 1))], n=a.n, n_rows_a=a.n, want=("a",))[0]


def _row_pred_counts(plan: JoinPlan, a: DeviceSide, b: DeviceSide, n_chrom: int, eng: HipEngine):
    """int64 device tensor: the ``b`` rows under the plan's predicate per ``a`` row (``_row_pred_matched``'s twin)."""
    if _ROW_PREDICATE_FORMS[("count", plan.predicate)]:
        try:
            return eng.count_pred(a, b, n_chrom, plan.predicate, plan.max_distance)
        except InvertedRows as exc:
            raise _inverted_rows_error(plan, exc) from exc
    import torch

    ra, _rb = _spatial_join(plan, a, b, n_chrom, eng)
    return torch.bincount(ra.long(), minlength=a.n)   # (plumbing: the pair ids are already reduced to one column)


def _pair_distances(plan: JoinPlan, lt, rt, a: DeviceSide, b: DeviceSide, ra, rb, eng: HipEngine) -> dict:
    """The plan's "pair_distance" projections -> ``{code: masked int64 array}``: DISTANCE of every pair
    ``(ra[i], rb[i])`` on the device (``HipEngine.distance``, the CASE of src/giql/expanders/_distance.py:67-117),
    NULLs as mask entries.  ``code`` = "lr" | "rl" (which table is the CASE's A operand) + "+signed" / "+stranded"."""
    import torch

    out: dict = {}
    codes = {p.column for p in plan.projection if p.side == "pair_distance"}
    strands = None
    for code in sorted(codes):
        parts = code.split("+")
        signed, stranded = "signed" in parts, "stranded" in parts
        if stranded and strands is None:
            ls, rs = (plan.strand_col or "strand,strand").split(",")
            strands = tuple(torch.from_numpy(_strand_codes(_column(t, c), 4)).to(eng.device)
                            for t, c in ((lt, ls), (rt, rs)))
        first, second, rows_1, rows_2 = (a, b, ra, rb) if parts[0] == "lr" else (b, a, rb, ra)
        s1, s2 = (strands if parts[0] == "lr" else strands[::-1]) if stranded else (None, None)
        dist, valid = eng.distance(first, second, rows_1.contiguous(), rows_2.contiguous(), signed=signed,
                                   stranded=stranded, strand_a=s1, strand_b=s2)
        out[code] = np.ma.masked_array(dist.cpu().numpy(), mask=(valid == 0).cpu().numpy())
    return out


def _computed_columns(plan: JoinPlan, lt, rt, a: DeviceSide, b: DeviceSide, ra, rb, eng: HipEngine) -> list:
    """The plan's computed columns (``JoinPlan.expressions``: bedtools -wo / -wao's ``overlap_bp``) for the final row
    ids ``(ra[i], rb[i])`` -- after the residual filters and after the pad of a LEFT join, whose rows carry
    ``rb == -1``: the kernel reads that as the right table's NULL row -- as int64 / float64 arrays, masked where the
    value is NULL.  All of them go through ``HipEngine.eval_exprs`` on the device; the raw ``start`` / ``end`` are
    there already, every other column is uploaded once (``_Residuals``)."""
    from .engine import expr_can_float

    res = _Residuals(plan, lt, rt, eng, dev_sides={"l": a, "r": b})
    trees = [res._spec(e, where="computed column") for e in plan.expressions]
    outs = eng.eval_exprs(trees, idx_a=ra.contiguous(), idx_b=rb.contiguous(), n_rows_a=a.n, n_rows_b=b.n)
    cols = []
    for tree, (vals, valid) in zip(trees, outs):
        v = vals.cpu().numpy().astype(np.float64 if expr_can_float(tree) else np.int64, copy=False)
        cols.append(v if valid is None else np.ma.masked_array(v, mask=(valid == 0).cpu().numpy()))
    return cols


def _join_with_residuals(plan: JoinPlan, lt, rt, a: DeviceSide, b: DeviceSide, n_chrom: int, eng: HipEngine):
    """INNER / SEMI / ANTI with residual predicates; returns device row ids.

    One-sided predicates shrink that side BEFORE the join, two-sided ones filter the
    pairs after it (what inlining them into the per-chromosome ON amounts to,
    intersects_duckdb.py:1239-1243).  For SEMI / ANTI only the ON residuals take part
    in the existence test; WHERE residuals filter the surviving left rows (#200,
    intersects_duckdb.py:1164-1177)."""
    rb_ = _Residuals(plan, lt, rt, eng, dev_sides={"l": a, "r": b})
    semi = plan.kind in ("SEMI", "ANTI")
    clauses = rb_.clauses(plan.residuals)   # every member of a clause comes from the same SQL clause
    joinside = [c for c in clauses if not (semi and c[0].clause == "where")]
    outer = [c for c in clauses if semi and c[0].clause == "where"]
    left_only = [c for c in joinside if rb_.sides(c) == {"l"}]
    right_only = [c for c in joinside if rb_.sides(c) == {"r"}]
    both = [c for c in joinside if rb_.sides(c) == {"l", "r"}]
    ids_a = eng.select(rb_.preds(left_only), n=a.n, n_rows_a=a.n, want=("a",))[0] if left_only else None
    ids_b = eng.select(rb_.preds(right_only), n=b.n, n_rows_b=b.n, want=("b",))[1] if right_only else None
    a_sub, b_sub = _subset(eng, a, ids_a), _subset(eng, b, ids_b)

    def globalise(rows, ids):
        return rows if ids is None else eng.take([ids], rows)[0]

    if not semi or both:
        ra, rb = _spatial_join(plan, a_sub, b_sub, n_chrom, eng)
        ra, rb = globalise(ra, ids_a), globalise(rb, ids_b)
        if both:
            ra, rb = eng.select(rb_.preds(both), idx_a=ra.contiguous(), idx_b=rb.contiguous(),
                                n_rows_a=a.n, n_rows_b=b.n)
        if not semi:
            return ra, rb
        matched = ra
    elif plan.predicate != "intersects":
        matched = globalise(_row_pred_matched(plan, a_sub, b_sub, n_chrom, eng, False), ids_a)
    else:
        matched = globalise(eng.semi_anti(a_sub, b_sub, n_chrom, False), ids_a)
    flags = eng.mark(matched.contiguous(), a.n)
    final = [(("a", flags), "=", ("lit", 0 if plan.kind == "ANTI" else 1))] + rb_.preds(outer)
    return eng.select(final, n=a.n, n_rows_a=a.n, want=("a",))[0]


def _null_right(spec, device):
    """A predicate of ``_Residuals.preds`` with every right-table column replaced by a one-row, all-NULL stand-in
    (same dtype, validity byte 0): what a padded row of a LEFT join offers the WHERE clause."""
    import torch

    if not isinstance(spec, tuple):
        return spec
    if len(spec) >= 2 and spec[0] == "b" and torch.is_tensor(spec[1]):
        return ("b", torch.zeros(1, dtype=spec[1].dtype, device=device), torch.zeros(1, dtype=torch.uint8, device=device))
    return tuple(_null_right(x, device) for x in spec)


def _left_join_rows(plan: JoinPlan, lt, rt, a: DeviceSide, b: DeviceSide, n_chrom: int, eng: HipEngine):
    """A LEFT plan's row ids ``(ra, rb)``, ``rb == -1`` on a padded row.

    The ON residuals take part in matching only, exactly as an INNER join's do (left-only ones restrict which left
    rows CAN match, right-only ones shrink the right table, two-sided ones filter the pairs); ``left_pad``
    then appends every one of the ``a.n`` left rows that kept no pair (measured faster than composing the same rows
    from ``mark``, ``select`` and a concatenation: DESIGN.md, "LEFT OUTER joins").  The WHERE residuals filter that result under
    three-valued logic: the matched pairs through ``select`` as they are, the padded rows through the SAME
    ``select`` against a one-row all-NULL right table."""
    import torch
    from dataclasses import replace

    on = tuple(r for r in plan.residuals if r.clause == "on")
    where = tuple(r for r in plan.residuals if r.clause != "on")
    inner = replace(plan, kind="INNER", residuals=on)
    if on:
        ra, rb = eng.left_pad_pairs(*_join_with_residuals(inner, lt, rt, a, b, n_chrom, eng), a.n)
    elif plan.predicate == "intersects":
        ra, rb = eng.left_join(a, b, n_chrom)      # (the pairs land in buffers with room for the pad)
    else:
        ra, rb = eng.left_pad_pairs(*_spatial_join(inner, a, b, n_chrom, eng), a.n)
    if not where:
        return ra, rb
    n_matched = int((rb >= 0).sum())      # (the padded rows are the tail)
    res = _Residuals(plan, lt, rt, eng, dev_sides={"l": a, "r": b})
    preds = res.preds(res.clauses(where))
    ka, kb = ra[:0], rb[:0]
    if n_matched:
        ka, kb = eng.select(preds, idx_a=ra[:n_matched], idx_b=rb[:n_matched], n_rows_a=a.n, n_rows_b=b.n)
    n_pad = int(ra.shape[0]) - n_matched
    if not n_pad:
        return ka, kb
    stand_in = [_null_right(p, eng.device) for p in preds]
    kp = eng.select(stand_in, idx_a=ra[n_matched:], idx_b=torch.zeros(n_pad, dtype=torch.int32, device=eng.device),
                    n_rows_a=a.n, n_rows_b=1, want=("a",))[0]
    return torch.cat([ka, kp]), torch.cat([kb, torch.full_like(kp, -1)])


def _abs_max(col) -> int:
    """``max(|min|, |max|)`` of an integer Arrow column; 0 for a column of NULLs alone."""
    import pyarrow.compute as pc

    mm = pc.min_max(col)
    lo, hi = mm["min"].as_py(), mm["max"].as_py()
    return 0 if lo is None else max(abs(lo), abs(hi))


def _check_int_sum(column: str, col, n_inputs: int | None = None, noun: str = "rows") -> None:
    """SUM / AVG over the integer Arrow column ``col`` accumulate in int64 on the device, where DuckDB sums into a
    128-bit integer: refuse the column when ``n_inputs * max(|min|, |max|)`` could reach 2^63 instead of wrapping.
    ``n_inputs`` values are summed at most: the column's rows under MERGE, a join's ``"pairs"`` (``noun``) over it."""
    n_inputs = len(col) if n_inputs is None else n_inputs
    bound = _abs_max(col)
    if n_inputs * bound >= 2**63:
        raise ValueError(f"SUM / AVG over column {column!r}: {n_inputs} {noun} of magnitude up to {bound} "
                         "can overflow the int64 sum; cast the column to a float type")


def _merge_aggregate_inputs(plan: JoinPlan, tbl, keep, eng: HipEngine):
    """The value columns of a MERGE plan's aggregates on the device, ``[(func, values, valid)]`` in the plan's order,
    and each column's Arrow type.  Columns go up once (``_Residuals._numeric``: types and validity bytes); when the
    WHERE kept a subset they are taken by ``keep`` there, so the merge's row ids and the values stay aligned."""
    import pyarrow as pa

    res = _Residuals(plan, tbl, None, eng)
    inputs, types, taken = [], [], {}
    for ag in plan.aggregates:
        if ag.func == "STRING_AGG":
            if ("utf8", ag.column) not in taken:
                taken[("utf8", ag.column)] = _string_agg_column(ag.column, _column(tbl, ag.column), keep, eng)
            inputs.append(("STRING_AGG",) + taken[("utf8", ag.column)] + (ag.separator,))
            types.append(pa.string())
            continue
        col = res._arrow("l", ag.column)
        t = col.type
        if not (pa.types.is_integer(t) or pa.types.is_floating(t)):
            raise ValueError(f"{ag.func}({ag.column}): column {ag.column!r} has type {t}; MERGE aggregates take "
                             "integer and floating-point columns")
        if ag.func in ("SUM", "AVG") and pa.types.is_integer(t):
            _check_int_sum(ag.column, col)
        if ag.column not in taken:
            vals, valid = res._numeric("l", ag.column)
            if keep is not None:
                vals = vals[keep.long()].contiguous()
                valid = None if valid is None else valid[keep.long()].contiguous()
            taken[ag.column] = (vals, valid)
        inputs.append((ag.func,) + taken[ag.column])
        types.append(t)
    return inputs, types


def _string_agg_column(name: str, col, keep, eng: HipEngine):
    """A STRING_AGG column on the device: ``(offsets int32, data uint8, validity bytes or None)``.  Arrow ``string``
    goes up as it lies in memory -- a sliced array keeps its offsets into the whole data buffer -- ``large_string`` and
    dictionary-of-string are cast to ``string`` on the host first (pyarrow raises when the column does not fit int32
    offsets); any other type is refused.  When the WHERE kept a subset the column is taken by ``keep`` on the device,
    so the merge's row ids and the values stay aligned."""
    import pyarrow as pa
    import torch

    if isinstance(col, pa.ChunkedArray):
        col = col.combine_chunks() if col.num_chunks != 1 else col.chunk(0)
    if not isinstance(col, pa.Array):
        col = pa.array(np.asarray(col))
    t = col.type
    if pa.types.is_large_string(t) or (pa.types.is_dictionary(t) and (pa.types.is_string(t.value_type)
                                                                      or pa.types.is_large_string(t.value_type))):
        col = col.cast(pa.string())
    elif not pa.types.is_string(t):
        raise ValueError(f"STRING_AGG({name}): column {name!r} has type {t}; STRING_AGG beside MERGE takes string "
                         "columns")
    bufs = col.buffers()
    n = len(col)
    if bufs[1] is None:   # (an empty array may carry no offsets buffer)
        off = np.zeros(n + 1, np.int32)
    else:
        off = np.frombuffer(bufs[1], dtype=np.int32, count=n + 1 + col.offset)[col.offset:]
    data = np.frombuffer(bufs[2], dtype=np.uint8) if bufs[2] is not None else np.zeros(0, np.uint8)
    off_dev = torch.from_numpy(np.ascontiguousarray(off)).to(eng.device)
    data_dev = torch.from_numpy(np.ascontiguousarray(data)).to(eng.device)
    valid = None
    if col.null_count:
        valid = torch.from_numpy(np.ascontiguousarray(
            col.is_valid().to_numpy(zero_copy_only=False).astype(np.uint8))).to(eng.device)
    if keep is not None:
        off_dev, data_dev = eng.take_utf8(off_dev, data_dev, keep)
        valid = None if valid is None else valid[keep.long()].contiguous()
    return off_dev, data_dev, valid


def _string_agg_array(offsets, data, valid):
    """One STRING_AGG result of ``HipEngine.merge_agg`` as a nullable Arrow ``string`` column."""
    import pyarrow as pa

    ok = valid.cpu().numpy()
    n = int(ok.shape[0])
    vbuf = None if ok.all() else pa.py_buffer(np.packbits(ok, bitorder="little").tobytes())
    return pa.Array.from_buffers(pa.string(), n, [vbuf, pa.py_buffer(_to_host(offsets.contiguous())),
                                                  pa.py_buffer(_to_host(data))], null_count=int(n - ok.sum()))


def _execute_cluster_merge(plan: JoinPlan, tables, eng: HipEngine, return_indices: bool):
    """CLUSTER / MERGE over one table (src/giql/expanders/cluster.py:81-300,
    src/giql/expanders/merge.py:62-330): partition ids = dictionary-encoded chrom
    (sorted, so MERGE's ``ORDER BY chrom, start`` is the kernel's output order) with
    the strand folded in when stranded; RAW coordinates, as the window SQL reads them."""
    import pyarrow as pa
    import torch

    side = plan.left
    if side.table not in tables:
        raise ValueError(f"table {side.table!r} was not provided")
    tbl = tables[side.table]
    if plan.aggregates and return_indices:
        raise ValueError("return_indices=True has no place for a MERGE plan's aggregates; ask for the table")
    def sorted_codes(name: str):
        """(sorted dictionary as a numpy array, codes): Arrow's hash for string columns, numpy.unique otherwise."""
        what = f"{side.table}.{name}"
        fast = _arrow_codes(_column(tbl, name), what)
        if fast is not None:
            (codes,), dictionary = _sorted_union_codes([fast])
            return np.asarray(dictionary, dtype=str if dictionary else "U1"), codes
        v = _to_numpy(_column(tbl, name), what)
        return np.unique(v.astype(str) if v.dtype.kind not in "iu" else v, return_inverse=True)

    start = _int32_column(_column(tbl, side.start_col), f"{side.table}.{side.start_col}")
    end = _int32_column(_column(tbl, side.end_col), f"{side.table}.{side.end_col}")
    chrom_dict, chrom_ids = sorted_codes(side.chrom_col)
    n_strand = 1
    part = chrom_ids.astype(np.int64)
    strand_dict = None
    if plan.stranded:
        strand_dict, strand_ids = sorted_codes(plan.strand_col)
        n_strand = max(len(strand_dict), 1)
        part = part * n_strand + strand_ids
    n_part = len(chrom_dict) * n_strand
    if n_part > 2**31 - 1:
        raise ValueError("too many (chrom, strand) partitions")
    dev_side = DeviceSide.from_numpy(part.astype(np.int32), start, end, device=eng.device)  # offsets 0: raw
    keep = None
    if plan.residuals:
        keep = eng.select(_Residuals(plan, tbl, None, eng).preds(plan.residuals), n=dev_side.n,
                          n_rows_a=dev_side.n, want=("a",))[0]
        dev_side = _subset(eng, dev_side, keep)

    preds = None
    if plan.cluster_predicate:
        # predicate := ... PREV(col): both operand sides read the SAME table (the rows the WHERE kept), the current
        # row through side "l", its sorted predecessor through side "r" (cluster.py:281-296, 587-640; MERGE hands
        # its predicate to the CLUSTER underneath, merge.py:201-210)
        ptbl = tbl if keep is None else _rows_of(tbl, keep.cpu().numpy())
        preds = _Residuals(plan, ptbl, ptbl, eng).preds(plan.cluster_predicate)
    if plan.kind == "CLUSTER":
        ids = eng.cluster(dev_side, n_part, plan.distance, preds=preds)
        if return_indices:
            return (keep.cpu().numpy() if keep is not None else np.arange(dev_side.n)), ids.cpu().numpy()
        is_arrow = isinstance(tbl, pa.Table)
        all_cols = list(tbl.column_names) if is_arrow else list(tbl.keys() if isinstance(tbl, dict) else tbl.columns)
        names, cols = [], []
        want = [c for p in plan.projection for c in (all_cols if p.side == "star" else [p.column]) if p.side != "cluster"]
        taken = None
        if keep is not None:
            taken = (_device_take(tbl, want, keep, eng) if is_arrow
                     else {c: np.asarray(_column(tbl, c))[keep.cpu().numpy()] for c in want})
        for p in plan.projection:
            if p.side == "cluster":
                names.append(p.name)
                cols.append(pa.array(ids.cpu().numpy(), type=pa.int64()))
                continue
            for c, out_name in ([(c, c) for c in all_cols] if p.side == "star" else [(p.column, p.name)]):
                names.append(out_name)
                cols.append(taken[c] if taken is not None else _column(tbl, c))
        arrays = [c if isinstance(c, (pa.Array, pa.ChunkedArray)) else pa.array(c) for c in cols]
        return pa.Table.from_arrays(arrays, names=names)

    agg_out = ()
    if plan.aggregates:
        agg_in, agg_types = _merge_aggregate_inputs(plan, tbl, keep, eng)
        try:
            merged = eng.merge_agg(dev_side, n_part, plan.distance, agg_in, preds=preds)
        except GiqlHipError as exc:
            over = re.search(r"string aggregate (\d+): output of (\d+) bytes", str(exc))
            if exc.code != GIQL_ERR_CAPACITY or not over:
                raise
            ag = [a for a in plan.aggregates if a.func == "STRING_AGG"][int(over.group(1))]
            raise ValueError(f"STRING_AGG({ag.column}) AS {ag.name}: at least {over.group(2)} bytes of output exceed "
                             "the 2^31 - 1 bytes of one string column") from None
        agg_out = merged[4:]
    else:
        merged = eng.merge(dev_side, n_part, plan.distance, preds=preds)
    c, s, e, cnt = (t.cpu().numpy() for t in merged[:4])
    def named(dictionary, codes):
        """The dictionary's values at ``codes`` as an Arrow column (a take on the Arrow side: a Python list of
        millions of strings took longer than the merge)."""
        if dictionary.dtype.kind in "US":
            return pa.array(dictionary.tolist(), pa.string()).take(pa.array(codes))
        return pa.array(dictionary[codes])

    cols = {side.chrom_col: named(chrom_dict, c // n_strand)}
    if plan.stranded:
        cols[plan.strand_col] = named(strand_dict, c % n_strand)
    cols[side.start_col] = pa.array(s, type=pa.int32())
    cols[side.end_col] = pa.array(e, type=pa.int32())
    for p in plan.projection:
        if p.side == "count":
            cols[p.name] = pa.array(cnt, type=pa.int64())
        elif p.side == "agg":
            ag = plan.aggregates[int(p.column)]
            if ag.func == "STRING_AGG":
                cols[p.name] = _string_agg_array(*agg_out[int(p.column)])
                continue
            vals, valid = agg_out[int(p.column)]
            arr = pa.array(vals.cpu().numpy(), mask=~valid.cpu().numpy())
            if ag.func in ("MIN", "MAX"):  # the column's own type (the device holds int64 / float64: exact)
                arr = arr.cast(agg_types[int(p.column)])
            cols[p.name] = arr
    out = pa.table(cols)
    if plan.stranded and out.num_rows:  # kernel order is (chrom, strand, start); SQL: ORDER BY chrom, start
        out = out.sort_by([(side.chrom_col, "ascending"), (side.start_col, "ascending")])
    if return_indices:
        return c, s, e, cnt
    return out


def _filter_chrom_codes(col, what: str):
    """A filter table's chromosome column as ``(int32 codes, the values the codes index, validity bytes or None)``.
    An Arrow string column keeps the codes of its own dictionary -- the array ``_arrow_codes`` caches for a pinned
    or immutable table, so that ``_device_side`` finds the table's device copy again -- with NULL rows encoded as
    ``""`` and flagged in the validity beside."""
    fast = _arrow_codes(col, what, nulls_as="")
    if fast is not None:
        import pyarrow as pa

        codes, values = fast
        arr = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
        valid = None
        if arr.null_count:
            valid = np.ascontiguousarray(arr.is_valid().to_numpy(zero_copy_only=False).astype(np.uint8))
        if codes.flags.writeable:
            codes.setflags(write=False)   # (shared by every later query over this table)
        return codes, list(values), valid
    raw = _to_numpy_obj(col)
    null = np.fromiter((v is None or (isinstance(v, float) and v != v) for v in raw), dtype=bool, count=raw.size)
    values, codes = np.unique(np.where(null, "", raw).astype(str), return_inverse=True)
    return (np.ascontiguousarray(codes, dtype=np.int32), values.tolist(),
            np.ascontiguousarray(~null, dtype=np.uint8) if null.any() else None)


def _range_set_answers(plan: JoinPlan, tbl, eng: HipEngine) -> list:
    """``HipEngine.range_set_any`` over a FILTER plan's table: the chromosome column is encoded once, the chromosomes
    the plan's ranges name join its dictionary (one no row carries gets a code past the table's own), the bounds take
    the table's coordinate encoding (``range_sets.bounds``) and the raw int32 columns go up as they are."""
    import pyarrow as pa
    import torch

    from .range_sets import bounds

    side = plan.left
    codes, values, chrom_valid = _filter_chrom_codes(_column(tbl, side.chrom_col), f"{side.table}.{side.chrom_col}")
    code_of = {v: i for i, v in enumerate(values)}
    for rs in plan.range_sets:
        for c, _lo, _hi in rs.ranges:
            code_of.setdefault(c, len(code_of))
    valid = [chrom_valid, None, None]
    cols = []
    for k, name in ((1, side.start_col), (2, side.end_col)):
        col = _column(tbl, name)
        if isinstance(col, (pa.Array, pa.ChunkedArray)) and col.null_count:
            valid[k] = np.ascontiguousarray(col.is_valid().to_numpy(zero_copy_only=False).astype(np.uint8))
            col = col.fill_null(0)
        cols.append(col)
    if valid[1] is None and valid[2] is None:
        dev = _device_side(tbl, side, codes, eng)     # (a pinned table's device copy is found again here)
    else:
        dev = DeviceSide.from_numpy(codes, _int32_column(cols[0], f"{side.table}.{side.start_col}"),
                                    _int32_column(cols[1], f"{side.table}.{side.end_col}"), side.encoding, device=eng.device)
    sets = []
    for rs in plan.range_sets:
        on_start, on_end = zip(*[bounds(rs.op, r, side.encoding) for r in rs.ranges])
        sets.append((rs.op, [code_of[c] for c, _lo, _hi in rs.ranges], on_start, on_end))
    valid_dev = [None if v is None else torch.from_numpy(v).to(eng.device) for v in valid]
    return eng.range_set_any(dev.chrom, dev.start, dev.end, sets, valid=valid_dev)


def _execute_filter(plan: JoinPlan, tables, eng: HipEngine, return_indices: bool):
    """Literal-range filter of one table (BASELINE config 1): the plan's comparisons run
    in the select kernel, the projected columns are gathered on the device."""
    import pyarrow as pa

    side = plan.left
    if side.table not in tables:
        raise ValueError(f"table {side.table!r} was not provided")
    tbl = tables[side.table]
    n = _n_rows(tbl)
    preds = _Residuals(plan, tbl, None, eng).preds(plan.residuals)
    if plan.range_sets:
        # each set is one more predicate: the kernel's three-valued answer as a uint8 operand with its validity,
        # kept where it is TRUE (``= 1``) or, under NOT, where it is FALSE (``= 0``); a NULL answer fails both
        answers = _range_set_answers(plan, tbl, eng)
        preds += [(("a", value, valid), "=", ("lit", 0 if rs.negated else 1), 0)
                  for rs, (value, valid) in zip(plan.range_sets, answers)]
    keep = eng.select(preds, n=n, n_rows_a=n, want=("a",))[0]
    if return_indices:
        return keep.cpu().numpy()
    is_arrow = isinstance(tbl, pa.Table)
    all_cols = list(tbl.column_names) if is_arrow else list(tbl.keys() if isinstance(tbl, dict) else tbl.columns)
    want = [c for p in plan.projection for c in (all_cols if p.side == "star" else [p.column])]
    taken = (_device_take(tbl, want, keep, eng) if is_arrow
             else {c: np.asarray(_column(tbl, c))[keep.cpu().numpy()] for c in want})
    names, cols = [], []
    for p in plan.projection:
        for c, out_name in ([(c, c) for c in all_cols] if p.side == "star" else [(p.column, p.name)]):
            names.append(out_name)
            cols.append(taken[c])
    arrays = [c if isinstance(c, (pa.Array, pa.ChunkedArray)) else pa.array(c) for c in cols]
    return pa.Table.from_arrays(arrays, names=names)


def _execute_disjoin(plan: JoinPlan, tables, eng: HipEngine, return_indices: bool):
    """DISJOIN (src/giql/expanders/disjoin.py:102-202): both tables on the device under one chromosome dictionary
    (uploaded or reused like a join's sides), ``HipEngine.disjoin``, then the target's projected columns gathered
    by the parent row on the device, with ``disjoin_chrom`` (the parent's chromosome), ``disjoin_start`` and
    ``disjoin_end`` (the target's declared encoding) appended.  Runs on one device."""
    import pyarrow as pa

    for side in (plan.left, plan.right):
        if side is not None and side.table not in tables:
            raise ValueError(f"table {side.table!r} was not provided")
    tt = tables[plan.left.table]
    rt = tables[plan.right.table] if plan.right is not None else None
    t_chrom = _column(tt, plan.left.chrom_col)
    if rt is None:
        ia, ib, dictionary = encode_chroms(t_chrom, t_chrom)
    else:
        ia, ib, dictionary = encode_chroms(t_chrom, _column(rt, plan.right.chrom_col))
    target = _device_side(tt, plan.left, ia, eng)
    reference = _device_side(rt, plan.right, ib, eng) if rt is not None else None
    try:
        parent, ds, de = eng.disjoin(target, reference, len(dictionary))
    except ValueError as exc:
        bad = plan.left.table if "target" in str(exc) or plan.right is None else plan.right.table
        raise ValueError(f"DISJOIN: table {bad!r} has a row with start > end ({exc})") from exc
    if return_indices:
        return parent.cpu().numpy(), ds.cpu().numpy(), de.cpu().numpy()
    is_arrow = isinstance(tt, pa.Table)
    all_cols = list(tt.column_names) if is_arrow else list(tt.keys() if isinstance(tt, dict) else tt.columns)
    want = [c for p in plan.projection for c in (all_cols if p.side == "star" else [p.column] if p.side == "l" else [])]
    if any(p.side == "star" or p.column == "disjoin_chrom" for p in plan.projection):
        want.append(plan.left.chrom_col)
    taken = {}
    if want:
        taken = (_device_take(tt, want, parent, eng) if is_arrow
                 else {c: np.asarray(_column(tt, c))[parent.cpu().numpy()] for c in dict.fromkeys(want)})
    appended = {"disjoin_chrom": lambda: taken[plan.left.chrom_col],
                "disjoin_start": lambda: pa.array(ds.cpu().numpy(), type=pa.int32()),
                "disjoin_end": lambda: pa.array(de.cpu().numpy(), type=pa.int32())}
    names, cols = [], []
    for p in plan.projection:
        if p.side == "star":
            items = [(c, c, None) for c in all_cols] + [(c, c, appended[c]) for c in appended]
        else:
            items = [(p.column, p.name, appended[p.column] if p.side == "disjoin" else None)]
        for c, out_name, make in items:
            names.append(out_name)
            cols.append(make() if make is not None else taken[c])
    arrays = [c if isinstance(c, (pa.Array, pa.ChunkedArray)) else pa.array(c) for c in cols]
    return _finish_outer(pa.Table.from_arrays(arrays, names=names), plan)


def _execute_disjoin_segments(plan: JoinPlan, tables, eng: HipEngine, return_indices: bool):
    """A self-mode DISJOIN plan answered from the target's coverage segments (``plan.segments``; lowered with
    ``disjoin_aggregates``): ``HipEngine.coverage`` on the one device side, then ``disjoin_chrom`` = the dictionary
    taken at the segments' chromosome ids, ``disjoin_start`` / ``disjoin_end`` int32 in the target's declared
    encoding and every ``COUNT(*)`` as int64 under its alias.  ``"runs"`` merges abutting segments of equal depth;
    ``"distinct"`` needs no depth.  ``return_indices=True``: the four numpy arrays (chromosome ids of the sorted
    dictionary, start, end, depth -- ``None`` for ``"distinct"``).  Runs on one device."""
    import pyarrow as pa
    from dataclasses import replace

    if plan.left.table not in tables:
        raise ValueError(f"table {plan.left.table!r} was not provided")
    tt = tables[plan.left.table]
    t_chrom = _column(tt, plan.left.chrom_col)
    ia, _ib, dictionary = encode_chroms(t_chrom, t_chrom)
    target = _device_side(tt, plan.left, ia, eng)
    with_depth = plan.segments != "distinct"
    try:
        c, s, e, d = eng.coverage(target, len(dictionary), runs=plan.segments == "runs", with_depth=with_depth)
    except ValueError as exc:
        raise ValueError(f"DISJOIN: table {plan.left.table!r} has a row with start > end ({exc})") from exc
    c, s, e = c.cpu().numpy(), s.cpu().numpy(), e.cpu().numpy()
    d = d.cpu().numpy() if d is not None else None
    if return_indices:
        return c, s, e, d
    names = pa.array(dictionary).take(pa.array(c))
    if isinstance(t_chrom, (pa.Array, pa.ChunkedArray)) and names.type != t_chrom.type:
        names = names.cast(t_chrom.type)      # the column's own type, as the gather of the ungrouped plan returns it
    made = {"disjoin_chrom": names, "disjoin_start": pa.array(s, type=pa.int32()),
            "disjoin_end": pa.array(e, type=pa.int32())}
    cols = [made[p.column] if p.side == "disjoin" else pa.array(d, type=pa.int64()) for p in plan.projection]
    out = pa.Table.from_arrays(cols, names=[p.name for p in plan.projection])
    return _finish_outer(out, replace(plan, distinct=False))   # (the segments are distinct already)


def _finish_count(plan, lt, rt, counts, n_chrom, eng, ia, return_indices, a_dev=None):
    """count_overlaps: COUNT(b.col) per distinct left key, zero-filled
    (src/giql/expanders/intersects_duckdb.py:806-854; oracle semantics of
    tests/test_duckdb_iejoin.py:66-81: a key held by k duplicate left rows counts
    k times its overlaps).  ``counts`` = the per-left-row overlap counts (``_join_piece``: a device tensor
    from one engine, a host array from the multi-device call); ``eng`` = the engine the GROUP BY may run
    on (``None``: on the host)."""
    import pyarrow as pa

    counts_dev = counts if hasattr(counts, "cpu") else None
    if counts_dev is not None:
        counts = None   # fetched below only if the host needs them

    cnt_proj = [p for p in plan.projection if p.side == "count"][0]
    ccol = _column(rt, cnt_proj.column)
    if hasattr(ccol, "null_count") and ccol.null_count:
        # COUNT(col) skips NULLs; the kernels count rows
        raise ValueError(f"COUNT({plan.right.alias}.{cnt_proj.column}) over a column with NULLs is not "
                         "supported by dialect='hip'")
    n_left = int((counts_dev if counts_dev is not None else counts).shape[0])
    if return_indices:
        return counts_dev.cpu().numpy() if counts_dev is not None else counts
    keys = [p for p in plan.projection if p.side == "l"]
    interval_cols = {plan.left.chrom_col, plan.left.start_col, plan.left.end_col}
    if eng is not None and {p.column for p in keys} == interval_cols and isinstance(lt, pa.Table) and n_left:
        # GROUP BY the left interval itself: grouped and summed on the GPU
        # (giql_hip_group_rows_dev / giql_hip_segment_sum_dev), keys gathered by the take kernel
        import torch

        a = a_dev if a_dev is not None else _device_side(lt, plan.left, ia, eng)   # (the join's own upload)
        try:
            gid, rep = eng.group_rows(a, n_chrom)
        except Exception as exc:  # (group_rows splits a genome wider than 32 bits itself: a safety net only)
            if getattr(exc, "code", None) != -5:
                raise
            gid = None
        if gid is not None:
            if counts_dev is None:
                counts_dev = torch.from_numpy(counts).to(eng.device)
            sums = eng.segment_sum(counts_dev, gid, int(rep.shape[0]))
            taken = _device_take(lt, [p.column for p in keys], rep, eng)
            cols = {p.name: taken[p.column] for p in keys}
            cols[cnt_proj.name] = pa.array(sums.cpu().numpy(), type=pa.int64())
            return pa.table(cols).select([p.name for p in plan.projection])
    if counts is None:
        counts = counts_dev.cpu().numpy()
    cols = {p.name: _column(lt, p.column) for p in keys}
    cols[cnt_proj.name] = pa.array(counts, type=pa.int64())
    tbl = pa.table({k: (v if isinstance(v, (pa.Array, pa.ChunkedArray)) else pa.array(v)) for k, v in cols.items()})
    if tbl.num_rows == 0:
        return tbl
    # other key sets (a subset of the interval columns, or extra payload columns): host GROUP BY
    out = tbl.group_by([p.name for p in keys], use_threads=False).aggregate([(cnt_proj.name, "sum")])
    out = out.rename_columns([cnt_proj.name if c == cnt_proj.name + "_sum" else c for c in out.column_names])
    return out.select([p.name for p in plan.projection])


# ------------------------------------------------------------- grouped aggregates over a join (the map shape)
def _aggregated_types(plan: JoinPlan, rt) -> dict:
    """``{column: Arrow type}`` of the right-table columns a plan's aggregates read (None: no such column)."""
    import pyarrow as pa

    types = {}
    for a in plan.aggregates:
        if a.side != "r" or a.column in types:
            continue
        try:
            col = _column(rt, a.column)
        except (KeyError, ValueError):
            types[a.column] = None
            continue
        t = getattr(col, "type", None)
        if t is None:
            try:
                t = pa.from_numpy_dtype(np.asarray(col).dtype)
            except (pa.ArrowNotImplementedError, TypeError):
                t = pa.string()    # (an object array: not a numeric column, whatever it holds)
        types[a.column] = t.value_type if pa.types.is_dictionary(t) else t
    return types


def _routes_join_aggregates(plan: JoinPlan, right_types: dict, return_indices: bool, devices) -> bool:
    """Whether ``execute`` answers a plan through ``_execute_join_aggregates``: a plan lowered in the map shape
    (``join_aggregates``; shape.is_map_shape) -- INNER, or LEFT with ON residuals only, grouped by left-side columns,
    every projected column a key, 1..8 aggregates that are COUNT(*), COUNT(<right column>) of any type, or SUM / AVG /
    MIN / MAX of a signed-integer or float32 / float64 right column (``right_types``: column -> Arrow type), or any of
    the five over an expression of the pair (side "x": the plan's expressions are exactly those such aggregates name)
    -- asked for as a table, on one device.  Anything else takes the path it takes without the flag."""
    import pyarrow as pa

    from .shape import MAP_AGG_MAX, map_aggregate_ok

    if not plan.join_aggregates or plan.kind not in ("INNER", "LEFT") or return_indices:
        return False
    if devices is not None and len(devices) > 1:
        return False
    if plan.kind == "LEFT" and any(r.clause != "on" for r in plan.residuals):
        return False
    if not plan.group_by or not 1 <= len(plan.aggregates) <= MAP_AGG_MAX:
        return False
    # expressions: only those that aggregates (side "x") refer to, and every one of them
    if {int(a.column) for a in plan.aggregates if a.side == "x"} != set(range(len(plan.expressions))):
        return False
    if any(p.side != "l" or p.column == "*" or p.name not in plan.group_by for p in plan.projection):
        return False
    for a in plan.aggregates:
        if not map_aggregate_ok(a.func, a.side, a.distinct):
            return False
        if a.side in ("*", "x"):
            continue
        t = right_types.get(a.column)
        if t is None:
            return False
        if a.func != "COUNT" and not (pa.types.is_signed_integer(t) or pa.types.is_float32(t) or pa.types.is_float64(t)):
            return False
    return True


def expression_abs_bound(tree, column_info):
    """An absolute bound of an integer expression tree (the plan's serialised form: ``[kind, value]`` leaves,
    ``["fn", op, [children]]``) by interval arithmetic, or None where the tree can yield a float -- a float sum does not
    wrap.  ``column_info(side, column) -> (max |value|, is_float)`` for the columns it reads.  ``+`` and ``-`` add the
    bounds, ``*`` multiplies them, NEG / ABS keep theirs, LEAST / GREATEST / a CASE take their largest argument (a
    CASE's condition does not count), a comparison or boolean is at most 1, NULL is 0; ``/`` is a float."""
    if tree[0] != "fn":
        kind, value = tree[0], tree[1]
        if kind == "int":
            return abs(int(value))
        if kind == "float":
            return None
        if kind == "str":
            return 0
        bound, is_float = column_info(kind, value)
        return None if is_float else int(bound)
    op, kids = tree[1], tree[2]
    if op == "null":
        return 0
    if op in ("=", "!=", "<", "<=", ">", ">=", "isnull", "notnull", "and", "or", "not"):
        return 1
    if op == "/":
        return None
    bounds = [expression_abs_bound(k, column_info) for k in (kids[1:] if op == "if" else kids)]
    if any(b is None for b in bounds):
        return None
    if op in ("+", "-"):
        return sum(bounds)
    if op == "*":
        out = 1
        for b in bounds:
            out *= b
        return out
    if op in ("neg", "abs", "least", "greatest", "if"):
        return max(bounds)
    raise ValueError(f"expression operator {op!r}")


def check_pair_expr_int_sum(name: str, tree, column_info, n_inputs: int) -> None:
    """SUM / AVG of an integer expression accumulate in int64: refuse, naming the aggregate, when ``n_inputs`` values
    of magnitude up to the tree's bound (``expression_abs_bound``) could reach 2^63, instead of wrapping.  A tree that
    can yield a float is exempt."""
    bound = expression_abs_bound(tree, column_info)
    if bound is not None and n_inputs * bound >= 2**63:
        raise ValueError(f"SUM / AVG in aggregate {name!r}: {n_inputs} values of magnitude up to {bound} can overflow "
                         "the int64 sum; make the expression a float (multiply by 1.0)")


def _column_info(res: "_Residuals"):
    """``column_info`` of ``expression_abs_bound`` over a plan's tables: (max |value| from the column's min / max,
    is it a float column); a column that is no number (a string under a comparison) counts 0."""
    import pyarrow as pa

    def info(side: str, column: str):
        col = res._arrow(side, column)
        if pa.types.is_floating(col.type):
            return 0, True
        if pa.types.is_boolean(col.type):
            return 1, False
        if not pa.types.is_integer(col.type):
            return 0, False
        return _abs_max(col), False
    return info


#: how an aggregate over expression <index> is keyed among the partials of ``_combine_join_partials``, which knows
#: right-table columns only (names beginning ``__giql_`` are the project's own)
_X_COLUMN = "__giql_x{}"


def _execute_join_aggregates(plan: JoinPlan, lt, rt, eng: HipEngine, pins: dict | None = None):
    """A map-shape plan (``_routes_join_aggregates``): the join's unpadded pairs, reduced per left row on the device
    (``HipEngine.pair_aggregate``: no gather per pair, nothing per pair comes to the host), then the per-row partials
    combined per distinct left key on the host over ``n_left`` rows (``_combine_join_partials``).  The pairs come from
    where the same join takes them without the flag: a pinned table's index (``_indexed_inner``) where one serves, else
    ``_spatial_join`` / ``_join_with_residuals``.  Returns the finished table, or None when the join yields 2^31 pairs
    or more (the caller takes the other path, which joins again).

    An aggregate over an expression (side "x"; the ``aggregate_expressions`` opt-in) goes to the same call as
    ``("expr", tree)``: the value is computed at the pair inside the reduction, no per-pair array exists.  SUM / MIN /
    MAX of it come back as int64 or float64 by the rule of the computed columns (``expr_can_float``).  Under a LEFT
    plan SQL evaluates the expression on the padded row of a left row without a pair too -- LEAST / GREATEST skip the
    NULLs, so ``SUM(LEAST(a.end, b.end) - GREATEST(a.start, b.start))`` of such a row is ``a.end - a.start``: those rows
    get one value each from ``eval_exprs`` (right id -1 = the NULL row), folded in as a partial of one input."""
    import pyarrow as pa
    from dataclasses import replace

    from .engine import expr_can_float

    # (an aggregate over an expression plays no part in finding the pairs)
    inner = replace(plan, kind="INNER", join_aggregates=False, expressions=(),
                    aggregates=tuple(a for a in plan.aggregates if a.side != "x"))
    got = None
    a = b = None
    if (plan.predicate == "intersects" and not plan.residuals and pins
            and any(p is not None and p.index for p in pins.values())):
        got = _indexed_inner(inner, lt, rt, pins, eng)   # (None: the index does not serve this pair of tables)
    if got is not None:
        ra, rb = got
    else:
        ia, ib, dictionary = encode_chroms(_column(lt, plan.left.chrom_col), _column(rt, plan.right.chrom_col))
        n_chrom = len(dictionary)
        a = _device_side(lt, plan.left, ia, eng)
        b = _device_side(rt, plan.right, ib, eng)
        if plan.residuals:
            ra, rb = _join_with_residuals(inner, lt, rt, a, b, n_chrom, eng)
        else:
            ra, rb = _spatial_join(inner, a, b, n_chrom, eng)
    n_left, n_right = _n_rows(lt), _n_rows(rt)
    n_pairs = int(ra.shape[0])
    if n_pairs >= 2**31:
        return None
    res = _Residuals(plan, lt, rt, eng, dev_sides={"l": a, "r": b})
    asked, slot, types = [], {}, {}   # the engine's aggregates, one per distinct (function, column); AVG asks for SUM
    trees = {}                        # expression index -> the engine's tree
    for ag in plan.aggregates:
        if ag.side == "*":
            continue
        func = "SUM" if ag.func == "AVG" else ag.func
        if ag.side == "x":            # equal (function, tree) are asked for once: equal trees share an index
            k, column = int(ag.column), _X_COLUMN.format(ag.column)
            if k not in trees:
                trees[k] = res._spec(plan.expressions[k], where="aggregate")
                types[column] = pa.float64() if expr_can_float(trees[k][1]) else pa.int64()
            if func == "SUM":
                unmatched = n_left if plan.kind == "LEFT" else 0     # (at most: every such row adds one input)
                check_pair_expr_int_sum(ag.name, plan.expressions[k].value, _column_info(res), n_pairs + unmatched)
            if (func, column) not in slot:
                slot[(func, column)] = len(asked)
                asked.append((func, trees[k]))
            continue
        if (func, ag.column) in slot:
            continue
        col = res._arrow("r", ag.column)
        types[ag.column] = col.type
        if func == "COUNT":
            entry = ("COUNT", None, res._valid(col))
        else:
            if func == "SUM" and pa.types.is_integer(col.type):
                _check_int_sum(ag.column, col, n_pairs, "pairs")
            entry = (func,) + res._numeric("r", ag.column)
        slot[(func, ag.column)] = len(asked)
        asked.append(entry)
    pairs, parts = eng.pair_aggregate(ra.contiguous(), rb.contiguous(), n_left, n_right, asked)
    partials = {key: (parts[j][0].cpu().numpy(), parts[j][1].cpu().numpy()) for key, j in slot.items()}
    pairs = pairs.cpu().numpy()
    if trees and plan.kind == "LEFT":
        partials = _fold_unmatched_rows(partials, trees, pairs, n_left, n_right, eng)
    # _combine_join_partials knows right-table columns: an aggregate over expression k reads "column" __giql_x<k>
    combine = replace(plan, expressions=(), aggregates=tuple(
        replace(a, side="r", column=_X_COLUMN.format(a.column)) if a.side == "x" else a for a in plan.aggregates))
    return _finish_grouped(_combine_join_partials(combine, lt, pairs, partials, types), plan)


def _fold_unmatched_rows(partials: dict, trees: dict, pairs: np.ndarray, n_left: int, n_right: int, eng: HipEngine):
    """A LEFT map-shape plan's aggregates over expressions: every left row without a pair contributes the expression's
    value on its padded row (right id -1: the NULL row) as a partial of ONE input -- the value and a non-NULL count of
    1, or NULL and 0.  ``partials``: ``(function, __giql_x<k>) -> (values, non-NULL counts)`` among others; ``trees``:
    ``k -> ("expr", tree)``."""
    import torch

    rows = np.flatnonzero(pairs == 0).astype(np.int32)
    if not rows.size:
        return partials
    idx_a = torch.from_numpy(rows).to(eng.device)
    order = sorted(trees)
    outs = eng.eval_exprs([trees[k] for k in order], idx_a=idx_a, idx_b=torch.full_like(idx_a, -1), n_rows_a=n_left,
                          n_rows_b=n_right)
    padded = {_X_COLUMN.format(k): (v.cpu().numpy(), None if ok is None else ok.cpu().numpy()) for k, (v, ok) in zip(order, outs)}
    return _fold_padded_values(partials, padded, rows)


def _fold_padded_values(partials: dict, padded: dict, rows: np.ndarray) -> dict:
    """``partials`` with the rows ``rows`` (no pair) of every aggregate over an expression set to one input each:
    ``padded``: ``__giql_x<k> -> (values, valid or None)`` of those rows.  COUNT is 1 where the value is not NULL."""
    out = dict(partials)
    for (func, column), (vals, nn) in partials.items():
        if column not in padded:
            continue
        v, ok = padded[column]
        ok = np.ones(rows.size, np.int64) if ok is None else (ok != 0).astype(np.int64)
        vals, nn = vals.copy(), nn.copy()
        nn[rows] = ok
        vals[rows] = ok if func == "COUNT" else np.where(ok != 0, v, 0).astype(vals.dtype)
        out[(func, column)] = (vals, nn)
    return out


def _combine_join_partials(plan: JoinPlan, lt, pairs: np.ndarray, partials: dict, types: dict):
    """The per-left-row partials of a map-shape plan combined per distinct left key, on the host with pyarrow over
    ``n_left`` rows: counts, sums and non-NULL counts add, MIN / MAX combine, AVG is ``double(total sum) / double(total
    non-NULL count)`` (NULL at 0).  ``pairs``: the pair count per left row; ``partials``: ``(function, right column) ->
    (values, non-NULL counts)`` as ``HipEngine.pair_aggregate`` returns them, AVG under SUM; ``types``: right column ->
    Arrow type (MIN / MAX come back in it).  INNER drops the keys whose rows have no pair; LEFT keeps them: COUNT(col)
    = 0, COUNT(*) = 1 per unmatched row (the padded row SQL counts), everything else NULL."""
    import pyarrow as pa
    import pyarrow.compute as pc

    keys = [p for p in plan.projection if p.side == "l"]
    cols = {p.name: _column(lt, p.column) for p in keys}
    cols = {k: (v if isinstance(v, (pa.Array, pa.ChunkedArray)) else pa.array(np.asarray(v))) for k, v in cols.items()}
    specs, finish = [], []      # pyarrow aggregations over the partial columns; how each output column is read
    for i, ag in enumerate(plan.aggregates):
        c = f"__giql_p{i}"
        if ag.side == "*":
            cols[c] = pa.array(np.maximum(pairs, 1) if plan.kind == "LEFT" else pairs, type=pa.int64())
            specs.append((c, "sum"))
            finish.append((ag, lambda t, c=c: t.column(c + "_sum")))
            continue
        vals, nn = partials[("SUM" if ag.func == "AVG" else ag.func, ag.column)]
        if ag.func == "COUNT":
            cols[c] = pa.array(nn, type=pa.int64())
            specs.append((c, "sum"))
            finish.append((ag, lambda t, c=c: t.column(c + "_sum")))
            continue
        null = nn == 0
        t_col = types[ag.column]
        if ag.func in ("SUM", "AVG"):
            cols[c] = pa.array(vals, mask=null)
            specs.append((c, "sum"))
            if ag.func == "SUM":
                finish.append((ag, lambda t, c=c: t.column(c + "_sum")))
            else:
                cols[c + "n"] = pa.array(nn, type=pa.int64())
                specs.append((c + "n", "sum"))
                # double(sum) / double(count), as the engine's AVG: an int64 sum past 2^53 rounds, it is no error
                finish.append((ag, lambda t, c=c: pc.divide(pc.cast(t.column(c + "_sum"), pa.float64(), safe=False),
                                                           pc.cast(t.column(c + "n_sum"), pa.float64()))))
            continue
        fn = ag.func.lower()
        if vals.dtype.kind != "f":
            cols[c] = pa.array(vals, mask=null)
            specs.append((c, fn))
            finish.append((ag, lambda t, c=c, fn=fn, ty=t_col: pc.cast(t.column(f"{c}_{fn}"), ty)))
            continue
        # a float MIN / MAX keeps the device's NaN order (NaN above every number) across the rows of a key: the
        # numbers combine by min / max, the NaNs by a flag -- MAX is NaN where any row's is, MIN only where no row
        # holds a number
        nan = np.isnan(vals) & ~null
        cols[c] = pa.array(vals, mask=null | nan)
        cols[c + "f"] = pa.array(nan.astype(np.int8))
        specs += [(c, fn), (c + "f", "max")]

        def read(t, c=c, fn=fn, ty=t_col):
            num, flag = t.column(f"{c}_{fn}"), pc.equal(t.column(c + "f_max"), 1)
            use_nan = flag if fn == "max" else pc.and_(flag, pc.is_null(num))
            return pc.cast(pc.if_else(use_nan, pa.scalar(float("nan"), pa.float64()), num), ty)
        finish.append((ag, read))
    tbl = pa.table(cols)
    if plan.kind == "INNER":
        tbl = tbl.filter(pa.array(pairs > 0))
    names = [p.name for p in keys]
    grouped = tbl.group_by(names, use_threads=False).aggregate(specs)   # use_threads=False: stable group order
    out = {n: grouped.column(n) for n in names}
    for ag, read in finish:
        out[ag.name] = read(grouped)
    order = list(plan.output) if plan.output else list(out)
    keep = [n for n in order if n in out] + [n for n in out if n not in order]
    return pa.Table.from_arrays([out[n] for n in keep], names=keep)


_PINNED_MIN_BYTES = 64 << 20
# plan kinds execute() answers from a pinned right table's index without sorting either side, and the index forms it
# does so for.  Both forms are on because both measured faster than the ordinary operators for all three kinds
# (tools/index_rows_timing.py, profiles/index_rows_timing.json.log: 1M x 10M, 2.1-2.3x fixed-length, 1.35-1.9x general;
# DESIGN.md "Row operators against an index"); a form that loses is switched off here and falls to the ordinary path.
_INDEXED_ROW_KINDS = ("COUNT", "SEMI", "ANTI")
_INDEXED_ROW_FORMS = {"fixed_length": True, "general": True}
# NEAREST (k = 1, unstranded) against a pinned right table's index, per index form: a form is on only where the
# indexed call measured faster than the ordinary one at BOTH sizes of tools/index_nearest_timing.py (1M x 10M and
# 10M x 10M) by more than the spread of its repetitions (profiles/index_nearest_timing.json.log; DESIGN.md "NEAREST
# against an index").  Measured: 3.4x (fixed-length) and 2.1x (general) at 1M x 10M, but 0.91x and 0.51x at 10M x 10M,
# so both forms are off.  A form that is off stays available through HipEngine.nearest_indexed.
_INDEXED_NEAREST_FORMS = {"fixed_length": False, "general": False}


def _to_host(t) -> np.ndarray:
    """A device tensor as a numpy array.  Large results travel through page-locked memory from torch's caching
    host allocator (a pageable 1.6 GB copy runs at ~11 GB/s, a pinned one at the link's ~55); the array -- and the
    Arrow column that wraps it -- keeps the block, which returns to the allocator's cache when released."""
    import torch

    if not t.is_cuda or t.numel() * t.element_size() < _PINNED_MIN_BYTES:
        return t.cpu().numpy()
    host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    host.copy_(t, non_blocking=True)
    torch.cuda.current_stream(t.device).synchronize()
    return host.numpy()


#: what one ``giql_hip_take_utf8_plan_dev`` call accepts: int32 output offsets, at most 0x7FFFFFF0 rows
UTF8_MAX_BYTES = 0x7FFFFFFF
UTF8_MAX_ROWS = 0x7FFFFFF0


def plan_utf8_slices(lengths: np.ndarray, max_bytes: int = UTF8_MAX_BYTES,
                     max_rows: int = UTF8_MAX_ROWS) -> list[tuple[int, int]]:
    """Split the gathered rows of a string column, whose byte lengths are ``lengths``, into
    consecutive ``(row_lo, row_hi)`` slices of at most ``max_rows`` rows and ``max_bytes`` bytes
    each, every slice as long as the limits allow.  Empty input gives no slice; a single row
    longer than ``max_bytes`` is a ``ValueError``."""
    lengths = np.asarray(lengths)
    n = int(lengths.shape[0])
    if max_bytes < 1 or max_rows < 1:
        raise ValueError("max_bytes and max_rows must be positive")
    if n and int(lengths.min()) < 0:
        raise ValueError("negative string length")
    ends = np.cumsum(lengths, dtype=np.int64)   # ends[i]: bytes of rows [0, i]
    out = []
    lo = 0
    while lo < n:
        base = int(ends[lo - 1]) if lo else 0
        hi = min(int(np.searchsorted(ends, base + max_bytes, side="right")), lo + max_rows, n)
        if hi == lo:
            raise ValueError(f"row {lo} is {int(lengths[lo])} bytes: longer than a string column's "
                             f"{max_bytes}-byte limit")
        out.append((lo, hi))
        lo = hi
    return out


def _utf8_lengths(off_dev, idx_dev):
    """Byte length of every gathered row, on the device (int64; 0 for ``idx < 0`` and for an id past the
    column, which the take kernel itself refuses)."""
    import torch

    n_rows = int(off_dev.shape[0]) - 1
    if n_rows <= 0:     # (an empty column has one offset: nothing to index, every id is a padded row's -1 or refused)
        return torch.zeros(idx_dev.shape[0], dtype=torch.int64, device=idx_dev.device)
    ok = (idx_dev >= 0) & (idx_dev < n_rows)
    ix = torch.where(ok, idx_dev, 0).long()
    lens = off_dev[ix + 1].long() - off_dev[ix].long()
    return torch.where(ok, lens, 0)


def _device_take(table, names, idx_dev, eng: HipEngine, pad_null: bool = False):
    """Gather the projected columns ``names`` of ``table`` by the device-resident
    row ids ``idx_dev`` ON THE GPU (``giql_hip_take_dev`` / ``giql_hip_take_utf8_*``;
    the reference's outer SELECT, ``intersects_duckdb.py:1402-1644``).

    Fixed-width numeric columns go through one fused launch; utf8/binary columns
    through the two-call offsets+bytes take; a validity bitmap travels as a
    byte-per-row column.  Returns ``{name: pyarrow.Array}``; a string column whose gather exceeds
    what one take accepts (``UTF8_MAX_BYTES`` bytes, ``UTF8_MAX_ROWS`` rows) comes back as a
    ``pyarrow.ChunkedArray`` of the column's own type (``plan_utf8_slices``).  Column types the
    kernels do not cover (nested, dictionary, large_*) use ``pyarrow.take`` on
    the host ids -- boundary plumbing, no join arithmetic.

    ``pad_null`` (the right side of a LEFT plan): a row id of -1 yields NULL in every column, whether or not the
    source column has NULLs of its own (the take kernels write zero bytes / an empty string there).
    """
    import pyarrow as pa
    import torch

    dev = idx_dev.device
    out: dict = {}
    fixed: list[tuple[str, object, object]] = []   # (name, arrow type, numpy values)
    masks: dict[str, np.ndarray] = {}
    strings: list[tuple[str, object, pa.Array]] = []
    host: list[str] = []
    for name in dict.fromkeys(names):
        col = _column(table, name)
        if isinstance(col, pa.ChunkedArray):
            col = col.combine_chunks() if col.num_chunks != 1 else col.chunk(0)
        if not isinstance(col, pa.Array):
            col = pa.array(np.asarray(col))
        t = col.type
        if pa.types.is_integer(t) or pa.types.is_floating(t) and t.bit_width in (16, 32, 64):
            vals = col.fill_null(0).to_numpy(zero_copy_only=False) if col.null_count else col.to_numpy(zero_copy_only=False)
            fixed.append((name, t, np.ascontiguousarray(vals)))
        elif pa.types.is_string(t) or pa.types.is_binary(t):
            strings.append((name, t, col))
        else:
            host.append(name)
            continue
        if col.null_count:
            masks[name] = np.ascontiguousarray(col.is_valid().to_numpy(zero_copy_only=False).astype(np.uint8))
    n = int(idx_dev.shape[0])
    cols_dev = [torch.from_numpy(v).to(dev) for _, _, v in fixed]
    mask_names = list(masks)
    cols_dev += [torch.from_numpy(masks[m]).to(dev) for m in mask_names]
    taken = eng.take(cols_dev, idx_dev) if cols_dev else []
    valid = {m: taken[len(fixed) + i].cpu().numpy().astype(bool) for i, m in enumerate(mask_names)}
    pad = (idx_dev < 0).cpu().numpy() if pad_null and n else None
    if pad is not None and pad.any():
        for name in [f[0] for f in fixed] + [s_[0] for s_ in strings]:
            valid[name] = (valid[name] & ~pad) if name in valid else ~pad
    for (name, t, v), tk in zip(fixed, taken):
        arr = _to_host(tk)
        out[name] = pa.array(arr, type=t, mask=(~valid[name]) if name in valid else None)
    for name, t, col in strings:
        bufs = col.buffers()
        off = np.frombuffer(bufs[1], dtype=np.int32, count=len(col) + 1 + col.offset)[col.offset:]
        data = np.frombuffer(bufs[2], dtype=np.uint8) if bufs[2] is not None else np.zeros(0, np.uint8)
        off_dev = torch.from_numpy(np.ascontiguousarray(off)).to(dev)
        data_dev = torch.from_numpy(np.ascontiguousarray(data)).to(dev)
        # a gather past int32 offsets comes back in row slices that each fit, as chunks of the column's own type
        slices = [(0, n)]
        if n:
            lens = _utf8_lengths(off_dev, idx_dev)
            if n > UTF8_MAX_ROWS or int(lens.sum()) > UTF8_MAX_BYTES:
                slices = plan_utf8_slices(lens.int().cpu().numpy(), UTF8_MAX_BYTES, UTF8_MAX_ROWS)
            del lens
        chunks = []
        for lo, hi in slices:
            o_dev, d_dev = eng.take_utf8(off_dev, data_dev, idx_dev[lo:hi])
            vbuf = None
            nulls = 0
            if name in valid:
                vbuf = pa.py_buffer(np.packbits(valid[name][lo:hi], bitorder="little").tobytes())
                nulls = int((hi - lo) - valid[name][lo:hi].sum())
            chunks.append(pa.Array.from_buffers(t, hi - lo, [vbuf, pa.py_buffer(_to_host(o_dev)),
                                                             pa.py_buffer(_to_host(d_dev))], null_count=nulls))
            del o_dev, d_dev
        out[name] = chunks[0] if len(chunks) == 1 else pa.chunked_array(chunks, type=t)
    if host:
        idx_np = idx_dev.cpu().numpy()
        idx_h = pa.array(idx_np, type=pa.int64(), mask=(idx_np < 0) if pad_null else None)
        for name in host:
            out[name] = _column(table, name).take(idx_h)
    return out


def _rows_of(table, rows: np.ndarray):
    """The rows ``rows`` of a table (pyarrow.Table / dict of arrays / DataFrame), same container type."""
    try:
        import pyarrow as pa

        if isinstance(table, pa.Table):
            return table.take(pa.array(rows, type=pa.int64()))
    except ImportError:  # pragma: no cover
        pass
    if isinstance(table, dict):
        return {k: np.asarray(v)[rows] for k, v in table.items()}
    return table.iloc[rows]


def _strand_codes(col, null_code: int) -> np.ndarray:
    """'+' -> 0, '-' -> 1, '.' -> 2, '?' -> 3, NULL -> ``null_code`` (a NULL strand never equals anything)."""
    message = "stranded NEAREST: strands other than '+' / '-' / '.' / '?' are not supported by dialect='hip'"
    fast = _arrow_codes(col, "strand", nulls_as="\0null")
    if fast is not None:   # Arrow's hash: a handful of distinct values whatever the table's size
        codes, values = fast
        lut = np.array([null_code if v == "\0null" else "+-.?".find(v) if len(v) == 1 else -1 for v in values] or [0], np.int32)
        if codes.size and (lut[np.unique(codes)] < 0).any():
            raise ValueError(message)
        return np.ascontiguousarray(lut[codes]) if len(values) else np.zeros(0, np.int32)
    v = np.asarray(_to_numpy_obj(col), dtype=object)
    out = np.full(v.shape[0], null_code, np.int32)
    for code, sym in enumerate("+-.?"):
        out[v == sym] = code
    bad = ~np.isin(out, (0, 1, 2, 3)) & np.array([x is not None for x in v], dtype=bool)
    if bad.any():
        raise ValueError(message)
    return out


def _nearest_rows(plan: JoinPlan, a: DeviceSide, b: DeviceSide, n_chrom: int, eng: HipEngine):
    """NEAREST of two device sides -> ``(rows_a, rows_b, distance)`` (device int32, device int32, host
    int64): one entry per result row, A rows ascending, a row's k matches in the reference's order
    ``ABS(distance), start, end`` (nearest.py:387-396).  A rows whose chromosome has no target row
    yield no row."""
    import torch

    if plan.k == 1:
        ib_dev, dist = eng.nearest(a, b, n_chrom, signed=plan.signed, max_distance=plan.max_distance)
        keep = torch.nonzero(ib_dev >= 0).flatten().to(torch.int32)
        return keep, ib_dev[keep.long()].contiguous(), dist[keep.long()].cpu().numpy()
    ib_k, dist_k = eng.nearest_k(a, b, n_chrom, plan.k, signed=plan.signed, max_distance=plan.max_distance)
    hit = torch.nonzero(ib_k >= 0)
    return (hit[:, 0].to(torch.int32).contiguous(), ib_k[hit[:, 0], hit[:, 1]].contiguous(),
            dist_k[hit[:, 0], hit[:, 1]].cpu().numpy())


def _chrom_values(col):
    """A chrom column as ``(int32 codes, values)`` in the column's OWN dictionary (sorted values)."""
    fast = _arrow_codes(col, "chrom column")
    if fast is not None:
        (codes,), dictionary = _sorted_union_codes([fast])
        return codes, list(dictionary)
    x = _to_numpy(col, "chrom column")
    if x.dtype.kind in "iu":
        dictionary, inverse = np.unique(x, return_inverse=True)
        return np.ascontiguousarray(inverse.astype(np.int32)), dictionary.tolist()
    _refuse_null_chroms(x)
    dictionary, inverse = np.unique(x.astype(str), return_inverse=True)
    return np.ascontiguousarray(inverse.astype(np.int32)), dictionary.tolist()


def _chrom_lookup(index_values, query_values) -> np.ndarray:
    """Position of each of a query table's chrom values in an index's dictionary (``len(index_values)``: no such
    chromosome), both as ``_chrom_values`` returns them.  Matched as :func:`encode_chroms` matches the two columns of
    an ordinary join: integers as integers (never negative) when both columns hold integers, otherwise as ``str``
    -- an int column joins a string column on ``str(id)``."""
    def ints(values):
        return all(isinstance(v, int) and not isinstance(v, bool) for v in values)

    both_int = ints(index_values) and ints(query_values)
    if both_int and any(v < 0 for v in (*index_values, *query_values)):
        raise ValueError("integer chrom ids must be non-negative")
    key = (lambda v: v) if both_int else str
    pos = {key(v): i for i, v in enumerate(index_values)}
    return np.fromiter((pos.get(key(v), len(index_values)) for v in query_values), dtype=np.int32,
                       count=len(query_values))


def _pinned_index(pin_, it, iside: PlanSide, eng: HipEngine):
    """``(DeviceIndex | None, dictionary)`` of a table pinned with ``index=True``: built on first use, ONE per
    (device, interval columns, encoding) -- the INNER join and the per-row operators share it.  ``None``: the
    table does not take the indexed form (remembered: it is not tried again)."""
    from . import _lib

    key = (str(eng.device), iside.chrom_col, iside.start_col, iside.end_col, iside.encoding)
    if key not in pin_._indexes:
        codes, dictionary = _chrom_values(_column(it, iside.chrom_col))
        try:
            dev = DeviceSide.from_numpy(codes, _int32_column(_column(it, iside.start_col), iside.start_col),
                                        _int32_column(_column(it, iside.end_col), iside.end_col), iside.encoding,
                                        device=eng.device)
            pin_._indexes[key] = (eng.index_create(dev, len(dictionary)), dictionary)
            del dev            # (the index holds its own arrays: the columns' device copy is not kept)
        except _lib.GiqlHipError as exc:
            if exc.code != _lib.GIQL_ERR_STATE:
                raise
            pin_._indexes[key] = (None, dictionary)    # this table does not take the indexed form
    return pin_._indexes[key]


def _index_query_side(qt, qside: PlanSide, dictionary, eng: HipEngine, own: bool = False):
    """A query table on the device with its chrom ids in an index's dictionary (the index speaks its OWN
    dictionary: it outlives the pairing of one query; chromosomes it lacks all get the id ``len(dictionary)`` and
    match nothing).  ``own=True`` also returns the same rows with ids from the query table's own dictionary and
    that dictionary's size -- what a GROUP BY over the query rows needs: the looked-up ids merge every chromosome
    the index lacks into one."""
    qcodes, qvalues = _chrom_values(_column(qt, qside.chrom_col))
    lut = _chrom_lookup(dictionary, qvalues)
    q = DeviceSide.from_numpy(lut[qcodes] if len(qvalues) else qcodes,
                              _int32_column(_column(qt, qside.start_col), qside.start_col),
                              _int32_column(_column(qt, qside.end_col), qside.end_col), qside.encoding, device=eng.device)
    if not own:
        return q
    import torch

    own_ids = torch.from_numpy(np.ascontiguousarray(qcodes, dtype=np.int32)).to(eng.device)
    return q, DeviceSide(own_ids, q.start, q.end, q.start_off, q.end_off), qcodes, len(qvalues)


def _indexed_inner(plan: JoinPlan, lt, rt, pins, eng: HipEngine):
    """INNER join through a pinned table's index, or None when no side offers one / the tables do not take the
    indexed form (the ordinary join follows).  The index speaks its OWN chromosome dictionary (it outlives the
    pairing of this query): the other table's chrom values are looked up in it, unknown ones match nothing."""
    from . import _lib

    for which in ("r", "l"):       # the right table first: the usual place of the large one
        pin_ = pins.get(which)
        if pin_ is None or not pin_.index:
            continue
        it, iside = (rt, plan.right) if which == "r" else (lt, plan.left)
        qt, qside = (lt, plan.left) if which == "r" else (rt, plan.right)
        index, dictionary = _pinned_index(pin_, it, iside, eng)
        if index is None:
            continue
        q = _index_query_side(qt, qside, dictionary, eng)
        try:
            rq, ri = eng.inner_join_indexed(q, index)
        except _lib.GiqlHipError as exc:
            if exc.code != _lib.GIQL_ERR_STATE:
                raise
            continue               # e.g. irregular query rows: the ordinary join answers them
        return (rq, ri) if which == "r" else (ri, rq)
    return None


def _indexed_rows(plan: JoinPlan, lt, rt, pin_, eng: HipEngine):
    """COUNT / SEMI / ANTI of the left table over the RIGHT table's index (the table pinned with ``index=True``), or
    None when the table does not take the indexed form or the left table holds irregular rows (the ordinary
    operator follows).  The right table's columns are not uploaded.  COUNT: ``(counts, left side, left ids,
    n_chrom)`` -- the per-left-row counts and the left side under its own dictionary, for ``_finish_count``; SEMI /
    ANTI: the ascending left row ids."""
    from . import _lib

    index, dictionary = _pinned_index(pin_, rt, plan.right, eng)
    if index is None or not _INDEXED_ROW_FORMS["general" if index.general else "fixed_length"]:
        return None
    try:
        if plan.kind == "COUNT":
            q, a_own, ia, n_chrom = _index_query_side(lt, plan.left, dictionary, eng, own=True)
            return eng.count_overlaps_indexed(q, index), a_own, ia, n_chrom
        q = _index_query_side(lt, plan.left, dictionary, eng)
        return eng.semi_anti_indexed(q, index, plan.kind == "ANTI")
    except _lib.GiqlHipError as exc:
        if exc.code != _lib.GIQL_ERR_STATE:
            raise
        return None                # irregular left rows: the ordinary operator answers them


def _routes_indexed_nearest(plan: JoinPlan, pins: dict, devices) -> bool:
    """Whether a plan is a candidate for ``_indexed_nearest``: NEAREST with k = 1, not stranded, on one device, its
    TARGET (right) table pinned with ``index=True`` (a pinned left table is of no use to it)."""
    return (plan.kind == "NEAREST" and plan.k == 1 and not plan.stranded and not plan.residuals
            and not (devices and len(devices) > 1) and pins.get("r") is not None and bool(pins["r"].index))


def _indexed_nearest(plan: JoinPlan, lt, rt, pin_, eng: HipEngine):
    """NEAREST k = 1 of the left table over the RIGHT table's index (the table pinned with ``index=True``): the
    ``(keep, ib_keep, distance)`` triple of ``_nearest_rows``, or None when the table does not take the indexed form,
    its index form is switched off (``_INDEXED_NEAREST_FORMS``) or the index declines NEAREST (a long run of rows on
    one start) -- the ordinary operator follows.  The right table's columns are not uploaded."""
    from . import _lib

    index, dictionary = _pinned_index(pin_, rt, plan.right, eng)
    if index is None or not _INDEXED_NEAREST_FORMS["general" if index.general else "fixed_length"]:
        return None
    try:
        index.prepare_nearest()    # (once per index; a declined index answers at once, before the left table is uploaded)
        q = _index_query_side(lt, plan.left, dictionary, eng)
        ib_dev, dist = eng.nearest_indexed(q, index, signed=plan.signed, max_distance=plan.max_distance)
    except _lib.GiqlHipError as exc:
        if exc.code != _lib.GIQL_ERR_STATE:
            raise
        return None
    import torch

    keep = torch.nonzero(ib_dev >= 0).flatten().to(torch.int32)
    return keep, ib_dev[keep.long()].contiguous(), dist[keep.long()].cpu().numpy()


def _join_piece(plan: JoinPlan, lt, rt, ia: np.ndarray, ib: np.ndarray, n_chrom: int, eng: HipEngine,
                return_indices: bool, device_projection: bool, sides_out: dict | None = None):
    """The join of ``lt`` x ``rt`` (chrom ids ``ia`` / ``ib`` from one shared dictionary) on ONE engine,
    up to but not including the outer clauses: the raw indices (``return_indices``), the per-left-row
    counts (COUNT), or the projected Arrow table before ``_finish_outer``.  ``execute`` runs it once;
    ``execute(devices=[...])`` once per device on that device's chromosomes."""
    import torch

    if plan.kind == "NEAREST" and plan.stranded:
        # stranded := true: a target row matches only on the reference row's strand (nearest.py:313-333).
        # Rows of different strands never pair and NULL strands match nothing, so the '+' and the '-' rows
        # are two independent NEAREST problems on the same chromosomes (folding the strand into the
        # chromosome id instead would double the linearised span: a whole genome with reads on both strands
        # is ~6.2e9 > 2^32); the distance of a '-' reference row flips its sign
        # (_distance.py:88-117).
        ls, rs = (plan.strand_col or "strand,strand").split(",")
        ca, cb = _strand_codes(_column(lt, ls), 4), _strand_codes(_column(rt, rs), 5)
        sa = _int32_column(_column(lt, plan.left.start_col), f"{plan.left.table}.{plan.left.start_col}")
        ea = _int32_column(_column(lt, plan.left.end_col), f"{plan.left.table}.{plan.left.end_col}")
        sb = _int32_column(_column(rt, plan.right.start_col), f"{plan.right.table}.{plan.right.start_col}")
        eb = _int32_column(_column(rt, plan.right.end_col), f"{plan.right.table}.{plan.right.end_col}")
        parts = []
        for code, sign in ((0, 1), (1, -1)):
            ra_, rb_ = np.nonzero(ca == code)[0], np.nonzero(cb == code)[0]
            if not ra_.size or not rb_.size:
                continue
            a = DeviceSide.from_numpy(ia[ra_], sa[ra_], ea[ra_], plan.left.encoding, device=eng.device)
            b = DeviceSide.from_numpy(ib[rb_], sb[rb_], eb[rb_], plan.right.encoding, device=eng.device)
            keep, ib_keep, dn = _nearest_rows(plan, a, b, n_chrom, eng)
            parts.append((ra_[keep.cpu().numpy()], rb_[ib_keep.cpu().numpy()], np.ma.masked_array(dn * sign, mask=False)))
        # '.' / '?' strands: the strand filter pairs such a reference row with the targets of ITS strand symbol, and the
        # distance CASE yields NULL for every one of them (_distance.py:88-117) -- so the ORDER BY falls through to
        # (start, end): the row's k targets are the first k of its chromosome in that order, distance NULL; under
        # max_distance there is none (NULL <= d is not true).  "First k by (start, end)" is asked of the NEAREST
        # kernel itself: one probe row per chromosome placed below every target sees them all downstream, nearest
        # = smallest start first, ties by (start, end) -- the same order.
        for code in (2, 3):
            ra_, rb_ = np.nonzero(ca == code)[0], np.nonzero(cb == code)[0]
            if not ra_.size or not rb_.size or plan.max_distance is not None:
                continue
            chroms = np.unique(ib[rb_])
            lo = int(sb[rb_].min()) - 2
            probe = DeviceSide.from_numpy(chroms.astype(np.int32), np.full(chroms.size, lo, np.int32),
                                          np.full(chroms.size, lo + 1, np.int32), plan.right.encoding, device=eng.device)
            b = DeviceSide.from_numpy(ib[rb_], sb[rb_], eb[rb_], plan.right.encoding, device=eng.device)
            if plan.k == 1:
                first = eng.nearest(probe, b, n_chrom)[0].cpu().numpy().reshape(-1, 1)
            else:
                first = eng.nearest_k(probe, b, n_chrom, plan.k)[0].cpu().numpy()
            slot = np.full(int(n_chrom), -1, np.int64)
            slot[chroms] = np.arange(chroms.size)
            rows = slot[ia[ra_]]                      # the probe row of each reference row's chromosome (-1: no target there)
            ok = rows >= 0
            cand = first[rows[ok]]                    # [n, k] target rows (indices into rb_), -1 = fewer than k
            hit = cand >= 0
            ka_ = np.repeat(ra_[ok], hit.sum(axis=1))
            parts.append((ka_, rb_[cand[hit]], np.ma.masked_array(np.zeros(ka_.size, np.int64), mask=True)))
        if parts:
            ka = np.concatenate([p[0] for p in parts])
            order = np.argsort(ka, kind="stable")   # A rows ascending; a row's k matches keep their order
            ka, kb = ka[order], np.concatenate([p[1] for p in parts])[order]
            dn = np.ma.concatenate([p[2] for p in parts])[order]
            if not np.ma.getmaskarray(dn).any():
                dn = np.asarray(dn.data)
        else:
            ka = kb = np.zeros(0, np.int64)
            dn = np.zeros(0, np.int64)
        if return_indices:
            return ka.astype(np.int32), kb.astype(np.int32), dn
        idx = {"l": torch.from_numpy(ka.astype(np.int32)).to(eng.device), "r": torch.from_numpy(kb.astype(np.int32)).to(eng.device)}
        return _project(plan, lt, rt, idx, {"distance": dn}, eng, device_projection)

    a = _device_side(lt, plan.left, ia, eng)
    b = _device_side(rt, plan.right, ib, eng)
    if sides_out is not None:     # (what the caller goes on with: COUNT's GROUP BY reads the left side again)
        sides_out["l"], sides_out["r"] = a, b
    if plan.kind == "COUNT":
        if plan.predicate != "intersects":
            return _row_pred_counts(plan, a, b, n_chrom, eng)
        return eng.count_overlaps(a, b, n_chrom)   # device int64, one per left row
    extra = {}
    if plan.kind == "INNER":
        if plan.residuals:
            ra, rb = _join_with_residuals(plan, lt, rt, a, b, n_chrom, eng)
        else:
            ra, rb = _spatial_join(plan, a, b, n_chrom, eng)
        if return_indices:
            return ra.cpu().numpy(), rb.cpu().numpy()
        idx = {"l": ra, "r": rb}
        if any(p.side == "pair_distance" for p in plan.projection):
            extra = {"pair_distance": _pair_distances(plan, lt, rt, a, b, ra, rb, eng)}
        if plan.expressions:
            extra["expr"] = _computed_columns(plan, lt, rt, a, b, ra, rb, eng)
    elif plan.kind == "LEFT":
        ra, rb = _left_join_rows(plan, lt, rt, a, b, n_chrom, eng)
        if return_indices:
            return ra.cpu().numpy(), rb.cpu().numpy()
        idx = {"l": ra, "r": rb}
        if plan.expressions:     # the padded rows go through the same call: their -1 is the right table's NULL row
            extra["expr"] = _computed_columns(plan, lt, rt, a, b, ra, rb, eng)
    elif plan.kind in ("SEMI", "ANTI"):
        if plan.residuals:
            rows = _join_with_residuals(plan, lt, rt, a, b, n_chrom, eng)
        elif plan.predicate != "intersects":
            rows = _row_pred_matched(plan, a, b, n_chrom, eng, plan.kind == "ANTI")
        else:
            rows = eng.semi_anti(a, b, n_chrom, plan.kind == "ANTI")
        if return_indices:
            return rows.cpu().numpy()
        idx = {"l": rows}
    else:  # NEAREST
        keep, ib_keep, dn = _nearest_rows(plan, a, b, n_chrom, eng)
        if return_indices:
            return keep.cpu().numpy(), ib_keep.cpu().numpy(), dn
        idx = {"l": keep, "r": ib_keep}
        extra = {"distance": dn}
    return _project(plan, lt, rt, idx, extra, eng, device_projection)


def _project(plan: JoinPlan, lt, rt, idx: dict, extra: dict, eng: HipEngine, device_projection: bool):
    """The plan's projected columns (+ the hidden carriers of ORDER BY / GROUP BY keys and aggregate
    arguments) gathered by the device-resident row ids -- the reference's outer SELECT
    (intersects_duckdb.py:1402-1644) -- as an Arrow table, before the outer clauses."""
    try:
        import pyarrow as pa
    except ImportError:  # pragma: no cover
        pa = None
    taken: dict = {}
    wanted = []
    for p in plan.projection:      # a.* / b.* beside a computed column: the table's columns, in its order
        if p.side in ("l", "r") and p.column == "*":
            tbl = lt if p.side == "l" else rt
            wanted += [Projection(p.side, c, c) for c in (tbl.column_names if hasattr(tbl, "column_names") else list(tbl))]
        else:
            wanted.append(p)
    wanted += [Projection(a.side, a.column, f"__giql_a{i}") for i, a in enumerate(plan.aggregates) if a.side in ("l", "r")]
    if pa is not None and device_projection and all(isinstance(t, pa.Table) for t in (lt, rt)):
        for s, tbl in (("l", lt), ("r", rt)):
            want = [p.column for p in wanted if p.side == s]
            if want and s in idx:
                taken[s] = _device_take(tbl, want, idx[s], eng, pad_null=(s == "r" and plan.kind == "LEFT"))
    idx_h = {s: v.cpu().numpy() for s, v in idx.items() if s not in taken}

    names, cols = [], []
    for p in wanted:
        names.append(p.name)
        if p.side == "distance":
            cols.append(extra["distance"])
        elif p.side == "pair_distance":
            cols.append(extra["pair_distance"][p.column])
        elif p.side == "expr":
            cols.append(extra["expr"][int(p.column)])
        elif p.side in taken:
            cols.append(taken[p.side][p.column])
        else:
            cols.append(_take(lt if p.side == "l" else rt, p.column, idx_h[p.side],
                              pad_null=(p.side == "r" and plan.kind == "LEFT")))
    if pa is None:  # pragma: no cover
        return dict(zip(names, cols))
    def as_arrow(c):
        if isinstance(c, (pa.Array, pa.ChunkedArray)):
            return c
        if isinstance(c, np.ma.MaskedArray):   # NULL distances ('.' / '?' strands under stranded := true)
            return pa.array(np.asarray(c.data), mask=np.ma.getmaskarray(c))
        return pa.array(c)

    arrays = [as_arrow(c) for c in cols]
    if not arrays:   # e.g. SELECT COUNT(*): no column to carry, only the row count
        n_rows = int(next(iter(idx.values())).shape[0])
        names, arrays = ["__giql_rows"], [pa.nulls(n_rows, pa.int8())]
    return pa.Table.from_arrays(arrays, names=names)


_SHARD_ENGINES: dict = {}


def _shard_engine(device: int, slot: int) -> HipEngine:
    """One context per (device, position in ``devices``): ``devices=[0, 0]`` is two contexts on one GPU."""
    key = (int(device), int(slot))
    if key not in _SHARD_ENGINES:
        _SHARD_ENGINES[key] = HipEngine(int(device))
    return _SHARD_ENGINES[key]


def _execute_sharded(plan: JoinPlan, lt, rt, ia, ib, n_chrom, devices, return_indices, device_projection):
    """``execute(..., devices=[d0, d1, ...])``: ONE process, one context and one host thread per entry of
    ``devices``.  Chromosomes are independent units of the join -- the reference partitions per chromosome
    and concatenates with UNION ALL (``_per_chrom.py:3-9, 46-74``) -- so they are LPT-packed onto the
    devices (``shard.plan_units``; a chromosome heavier than one device's share is cut by row ranges of
    its larger side, of A for the per-row operators), every device joins AND projects its own chromosomes,
    and the Arrow pieces are concatenated on the host: no index exchange at all.  The outer clauses
    (aggregates, DISTINCT, ORDER BY, LIMIT) then run once, on the whole result."""
    import threading

    from .distributed import unit_rows

    n_dev = len(devices)
    split_side = None if plan.kind == "INNER" else "a"
    shards = [unit_rows(ia, ib, n_chrom, n_dev, r, split_side=split_side) for r in range(n_dev)]
    pieces: list = [None] * n_dev
    errors: list = [None] * n_dev

    def work(r):
        try:
            rows_a, rows_b = shards[r]
            if rows_a.size == 0:
                return   # no left row, no result row (INNER / SEMI / ANTI / COUNT / NEAREST alike)
            eng = _shard_engine(devices[r], r)
            pieces[r] = _join_piece(plan, _rows_of(lt, rows_a), _rows_of(rt, rows_b), ia[rows_a], ib[rows_b], n_chrom,
                                    eng, return_indices, device_projection)
        except BaseException as exc:  # noqa: BLE001 -- re-raised on the caller's thread
            errors[r] = exc

    threads = [threading.Thread(target=work, args=(r,), name=f"giql-hip-dev{devices[r]}-{r}") for r in range(n_dev)]
    if os.environ.get("GIQL_EXECUTE_SERIAL"):   # debugging aid: the shards one after the other
        for r in range(n_dev):
            work(r)
        threads = []
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for e in errors:
        if e is not None:
            raise e
    have = [r for r in range(n_dev) if pieces[r] is not None]
    if plan.kind == "COUNT":
        counts = np.zeros(ia.shape[0], np.int64)
        for r in have:
            counts[shards[r][0]] = pieces[r].cpu().numpy()   # every A row lies in exactly one shard
        return counts
    if return_indices:
        if plan.kind == "INNER":
            ra = [shards[r][0][pieces[r][0]] for r in have]
            rb = [shards[r][1][pieces[r][1]] for r in have]
            cat = lambda xs: np.concatenate(xs).astype(np.int32) if xs else np.zeros(0, np.int32)  # noqa: E731
            return cat(ra), cat(rb)
        if plan.kind in ("SEMI", "ANTI"):
            rows = [shards[r][0][pieces[r]] for r in have]
            return np.sort(np.concatenate(rows)).astype(np.int32) if rows else np.zeros(0, np.int32)
        ka = np.concatenate([shards[r][0][pieces[r][0]] for r in have]) if have else np.zeros(0, np.int64)
        kb = np.concatenate([shards[r][1][pieces[r][1]] for r in have]) if have else np.zeros(0, np.int64)
        ds = [pieces[r][2] for r in have]   # (masked where the distance is NULL: '.' / '?' strands)
        dn = ((np.ma.concatenate(ds) if any(isinstance(x, np.ma.MaskedArray) for x in ds) else np.concatenate(ds))
              if have else np.zeros(0, np.int64))
        order = np.argsort(ka, kind="stable")
        return ka[order].astype(np.int32), kb[order].astype(np.int32), dn[order]
    import pyarrow as pa

    if not have:   # no left rows at all: an empty piece with the right schema from the first device
        return _join_piece(plan, _rows_of(lt, np.zeros(0, np.int64)), _rows_of(rt, np.zeros(0, np.int64)),
                           ia[:0], ib[:0], n_chrom, _shard_engine(devices[0], 0), False, device_projection)
    return pa.concat_tables([pieces[r] for r in have])


def execute(plan, tables, engine: HipEngine | None = None, *, giql_tables=None, return_indices=False,
            device_projection: bool = True, devices=None, outer_joins: bool = False, row_predicates: bool = False,
            select_expressions: bool = False, merge_aggregates: bool = False, range_sets: bool = False,
            string_aggregates: bool = False, join_aggregates: bool = False, disjoin_aggregates: bool = False,
            aggregate_expressions: bool = False):
    """Run *plan* (a :class:`JoinPlan`, its string form, or a GIQL query string; ``outer_joins``,
    ``row_predicates``, ``select_expressions``, ``merge_aggregates``, ``string_aggregates``, ``range_sets``,
    ``join_aggregates``, ``aggregate_expressions`` and ``disjoin_aggregates`` as in :func:`giql_amd.transpile.build_plan`, for a query string) against ``tables``
    (``{name: pyarrow.Table | dict of arrays}``).

    Returns a ``pyarrow.Table`` with the plan's projected columns (bag semantics,
    unspecified row order, as upstream), or ``{column: array}`` when pyarrow is
    absent.  ``return_indices=True`` returns the raw row indices instead:
    ``(row_a, row_b)`` for INNER and LEFT (``row_b == -1`` on a left row without a match), ``rows_a`` for SEMI/ANTI,
    ``(rows_a, idx_b, distance)`` for NEAREST (``distance`` a numpy masked array when
    ``stranded := true`` met '.' / '?' strands: those rows' distance is NULL) and the
    per-left-row counts for count_overlaps.  ``device_projection`` (default) gathers the projected columns
    on the GPU from the device-resident row ids; ``False`` ships the ids to the
    host and takes there.

    ``devices=[0, 1, ...]`` fans one call out over several GPUs of the node (one context and one host
    thread each; INNER / SEMI / ANTI / COUNT / NEAREST): the chromosomes are sharded over the devices,
    every device joins and projects its own, the pieces are concatenated (``_execute_sharded``).  One
    entry = that device; the single-table operators (CLUSTER / MERGE / literal-range FILTER) run on the
    first one.
    """
    relower = None   # a query string lowered with ``join_aggregates``: how to lower it again without the flag
    if isinstance(plan, str):
        if is_plan_string(plan):
            plan = JoinPlan.from_string(plan)
        else:
            query, opts = plan, dict(outer_joins=outer_joins, row_predicates=row_predicates,
                                     select_expressions=select_expressions, merge_aggregates=merge_aggregates,
                                     range_sets=range_sets, string_aggregates=string_aggregates,
                                     disjoin_aggregates=disjoin_aggregates)
            plan = build_plan(query, giql_tables, join_aggregates=join_aggregates,
                              aggregate_expressions=aggregate_expressions, **opts)
            relower = lambda: build_plan(query, giql_tables, **opts)  # noqa: E731
    if not isinstance(plan, JoinPlan):
        raise ValueError("plan must be a JoinPlan, a plan string or a GIQL query")
    devices = [int(d) for d in devices] if devices is not None else None
    if devices is not None and not devices:
        raise ValueError("devices must name at least one device")
    if engine is not None and devices is not None and len(devices) > 1:
        raise ValueError("pass either an engine or several devices, not both")
    eng = engine or default_engine(devices[0] if devices else 0)
    pinned = {name: t for name, t in tables.items() if isinstance(t, PinnedTable)}
    tables = {name: _unwrap(t) for name, t in tables.items()}   # (a pinned table stands for its Arrow table)
    if plan.kind in ("CLUSTER", "MERGE"):
        return _execute_cluster_merge(plan, tables, eng, return_indices)
    if plan.kind == "FILTER":
        return _execute_filter(plan, tables, eng, return_indices)
    if plan.kind == "DISJOIN":
        if plan.segments is not None:
            return _execute_disjoin_segments(plan, tables, eng, return_indices)
        return _execute_disjoin(plan, tables, eng, return_indices)
    for side in (plan.left, plan.right):
        if side.table not in tables:
            raise ValueError(f"table {side.table!r} was not provided")
    lt, rt = tables[plan.left.table], tables[plan.right.table]
    pins = {"l": pinned.get(plan.left.table), "r": pinned.get(plan.right.table)}
    if plan.join_aggregates:
        # the map shape: the join's pairs stay on the device and are aggregated per left row there
        got = None
        if _routes_join_aggregates(plan, _aggregated_types(plan, rt), return_indices, devices):
            got = _execute_join_aggregates(plan, lt, rt, eng, pins)
        if got is not None:
            return got
        if any(a.side == "x" for a in plan.aggregates):
            # no other path computes an aggregate over an expression
            raise ValueError("an aggregate over an expression runs in the map shape only: on one device, as a table "
                             "(not return_indices), over fewer than 2^31 pairs, a LEFT join without WHERE residuals")
        # outside the shape (a column type, return_indices, several devices) or 2^31 pairs and more: the query runs
        # -- or declines -- exactly as it does without the flag
        from dataclasses import replace
        plan = relower() if relower is not None else replace(plan, join_aggregates=False)
    if plan.expressions and devices is not None and len(devices) > 1:
        raise ValueError(f"a computed column is evaluated on one device; devices={devices!r} names {len(devices)}")
    if plan.kind == "LEFT" and devices is not None and len(devices) > 1:
        raise NotImplementedError(f"a LEFT OUTER join runs on one device; devices={devices!r} names {len(devices)} "
                                  "(the per-chromosome fan-out does not pad unmatched rows yet)")
    if plan.row_predicates and devices is not None and len(devices) > 1:
        raise NotImplementedError(f"SEMI / ANTI / COUNT over {plan.predicate.upper()} run on one device; "
                                  f"devices={devices!r} names {len(devices)}")
    if plan.predicate != "intersects" and devices is not None and len(devices) > 1:
        # one device, like DISJOIN: the per-chromosome fan-out shards an INTERSECTS join
        raise ValueError(f"{plan.predicate.upper()} joins run on one device; devices={devices!r} names {len(devices)}")
    has_pair_distance = any(p.side == "pair_distance" for p in plan.projection)
    if has_pair_distance and devices is not None and len(devices) > 1:
        raise ValueError(f"a DISTANCE column is computed on one device; devices={devices!r} names {len(devices)}")
    if (plan.kind == "INNER" and plan.predicate == "intersects" and not plan.residuals and not has_pair_distance
            and not plan.expressions and not (devices and len(devices) > 1)
            and any(p is not None and p.index for p in pins.values())):
        # a pinned table offers an index: the join reads it instead of spanning and sorting that table again
        got = _indexed_inner(plan, lt, rt, pins, eng)
        if got is not None:
            ra, rb = got
            if return_indices:
                return ra.cpu().numpy(), rb.cpu().numpy()
            return _finish_outer(_project(plan, lt, rt, {"l": ra, "r": rb}, {}, eng, device_projection), plan)
    if (plan.kind in _INDEXED_ROW_KINDS and plan.predicate == "intersects" and not plan.residuals
            and not (devices and len(devices) > 1) and pins["r"] is not None and pins["r"].index):
        # the per-row operators read the RIGHT table's index (a pinned left table is of no use to them): neither
        # side is sorted, the pinned table's columns are not uploaded
        got = _indexed_rows(plan, lt, rt, pins["r"], eng)
        if got is not None and plan.kind == "COUNT":
            counts, a_own, ia, n_chrom = got
            return _finish_count(plan, lt, rt, counts, n_chrom, eng, ia, return_indices, a_dev=a_own)
        if got is not None:
            if return_indices:
                return got.cpu().numpy()
            return _finish_outer(_project(plan, lt, rt, {"l": got}, {}, eng, device_projection), plan)
    if _routes_indexed_nearest(plan, pins, devices):
        # NEAREST k = 1 reads the RIGHT table's index: neither side is sorted, the pinned table's columns are not uploaded
        got = _indexed_nearest(plan, lt, rt, pins["r"], eng)
        if got is not None:
            keep, ib_keep, dn = got
            if return_indices:
                return keep.cpu().numpy(), ib_keep.cpu().numpy(), dn
            return _finish_outer(_project(plan, lt, rt, {"l": keep, "r": ib_keep}, {"distance": dn}, eng,
                                          device_projection), plan)
    ia, ib, dictionary = encode_chroms(_column(lt, plan.left.chrom_col), _column(rt, plan.right.chrom_col))
    n_chrom = len(dictionary)
    dev_sides: dict = {}
    if devices is not None and len(devices) > 1:
        piece = _execute_sharded(plan, lt, rt, ia, ib, n_chrom, devices, return_indices, device_projection)
    else:
        piece = _join_piece(plan, lt, rt, ia, ib, n_chrom, eng, return_indices, device_projection, sides_out=dev_sides)
    if plan.kind == "COUNT":
        return _finish_count(plan, lt, rt, piece, n_chrom, eng if not (devices and len(devices) > 1) else None,
                             ia, return_indices, a_dev=dev_sides.get("l"))
    if return_indices or isinstance(piece, dict):
        return piece
    return _finish_outer(piece, plan)


_PA_AGG = {"COUNT": "count", "SUM": "sum", "MIN": "min", "MAX": "max", "AVG": "mean"}


def _finish_outer(out, plan: JoinPlan):
    """The clauses that ride on the reference's outer SELECT wrapper (intersects_duckdb.py:1336-1400):
    aggregates / GROUP BY, DISTINCT, ORDER BY, OFFSET / LIMIT -- finished here on the projected Arrow
    table with pyarrow compute on the HOST (a first version: the join, the residual filters and the
    column gathers ran on the GPU; these operate on the already-reduced result)."""
    import pyarrow as pa

    if plan.aggregates:
        cols = {}
        # one aggregate at a time keeps the produced column names unambiguous
        keys = list(plan.group_by)
        base = None
        for i, a in enumerate(plan.aggregates):
            if a.side == "*":
                spec, produced = ([], "count_all"), "count_all"
            else:
                fn = "count_distinct" if (a.distinct and a.func == "COUNT") else _PA_AGG[a.func]
                spec, produced = (f"__giql_a{i}", fn), f"__giql_a{i}_{fn}"
            res = out.group_by(keys, use_threads=False).aggregate([spec])   # use_threads=False: stable group order
            if base is None:
                base = res
                for k in keys:
                    cols[k] = res.column(k)
            cols[a.name] = res.column(produced)
        order = list(plan.output) if plan.output else list(cols)
        keep = [n for n in order if n in cols] + [n for n in cols if n not in order]
        out = pa.Table.from_arrays([cols[n] for n in keep], names=keep)
    elif plan.group_by:   # GROUP BY without an aggregate: one row per key
        out = out.group_by(list(plan.group_by), use_threads=False).aggregate([])
        if plan.output:
            out = out.select([n for n in plan.output if n in out.column_names] +
                             [n for n in out.column_names if n not in plan.output])
    return _finish_grouped(out, plan)


def _finish_grouped(out, plan: JoinPlan):
    """The tail of :func:`_finish_outer` on a table that is aggregated already (or needs no aggregation): HAVING,
    DISTINCT, ORDER BY, OFFSET / LIMIT, and the hidden ``__giql_*`` columns dropped."""
    import pyarrow as pa

    if plan.having:
        import pyarrow.compute as pc

        cmp = {"=": pc.equal, "!=": pc.not_equal, "<": pc.less, "<=": pc.less_equal, ">": pc.greater,
               ">=": pc.greater_equal}
        mask, clause, prev = None, None, 0
        for h in list(plan.having) + [None]:
            if h is None or not (h.group and h.group == prev):    # a clause ends: AND it in
                if clause is not None:
                    mask = clause if mask is None else pc.and_kleene(mask, clause)
                clause = None
            if h is None:
                break
            lhs, rhs = (out.column(o.value) if o.kind == "name" else pa.scalar(o.value) for o in (h.lhs, h.rhs))
            m = (pc.is_null(lhs) if h.op == "isnull" else pc.is_valid(lhs)) if h.op in ("isnull", "notnull") \
                else cmp[h.op](lhs, rhs)
            clause = m if clause is None else pc.or_kleene(clause, m)   # members of one group are OR-ed
            prev = h.group
        out = out.filter(mask)   # NULL comparisons drop the group, as SQL's HAVING does
    visible = [n for n in out.column_names if not n.startswith("__giql_")]
    if plan.distinct:
        if plan.order_by and any(o[0] not in visible for o in plan.order_by):
            raise ValueError("ORDER BY a column that DISTINCT does not keep")
        out = out.select(visible).group_by(visible, use_threads=False).aggregate([])
    if plan.order_by:
        import pyarrow.compute as pc

        # per-key NULL placement: a validity flag sorted ahead of each key (pyarrow's own null_placement
        # is one setting for all the keys)
        keys, tmp = [], out
        for i, (n, desc, nulls_first) in enumerate(plan.order_by):
            flag = f"__giql_n{i}"
            tmp = tmp.append_column(flag, pc.is_null(tmp.column(n)))
            keys.append((flag, "descending" if nulls_first else "ascending"))   # True (NULL) first / last
            keys.append((n, "descending" if desc else "ascending"))
        out = out.take(pc.sort_indices(tmp, sort_keys=keys))
    if plan.offset is not None or plan.limit is not None:
        start = plan.offset or 0
        out = out.slice(start, plan.limit) if plan.limit is not None else out.slice(start)
    # (by position: a.* and b.* beside a computed column may carry one name twice)
    return out.select([i for i, n in enumerate(out.column_names) if not n.startswith("__giql_")])
