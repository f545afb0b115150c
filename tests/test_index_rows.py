"""The per-row operators against a table index (giql_hip_index_prepare_rows_dev / giql_hip_count_indexed_dev /
giql_hip_semi_anti_indexed_dev): the part of their C ABI that needs no GPU -- the symbols are exported, bound and
declared, and a NULL context or a NULL index is refused before a device is touched.  The results are checked on the
GPU (test_index_rows_gpu.py)."""

import ctypes
import os
import re

from giql_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("giql_hip_index_prepare_rows_dev", "giql_hip_count_indexed_dev", "giql_hip_semi_anti_indexed_dev")


def test_the_three_symbols_are_exported_bound_and_declared():
    L = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "giql_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(L, name), name
        assert name in _lib.SYMBOLS, name
        assert getattr(L, name).argtypes, name          # bound with argtypes
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert L.giql_hip_abi_version() == 4                # symbols were added, no struct changed


def test_a_null_context_or_index_is_invalid_without_a_device():
    L = _lib.load()
    side = _lib.CSide(None, None, None, 0, 0, 0)
    n = ctypes.c_int64(-1)
    fake = ctypes.create_string_buffer(64)              # stands for a non-NULL handle: it must not be looked into
    h = ctypes.cast(fake, ctypes.c_void_p)
    for ctx, idx in ((None, None), (None, h), (h, None)):
        assert L.giql_hip_index_prepare_rows_dev(ctx, idx, None) == _lib.GIQL_ERR_INVALID
        assert L.giql_hip_count_indexed_dev(ctx, idx, ctypes.byref(side), None, None) == _lib.GIQL_ERR_INVALID
        assert L.giql_hip_semi_anti_indexed_dev(ctx, idx, ctypes.byref(side), 0, None, ctypes.byref(n),
                                                None) == _lib.GIQL_ERR_INVALID
        assert b"NULL" in L.giql_hip_last_error()
    assert n.value == -1                                # nothing was written
