"""NEAREST (k = 1) against a table index (giql_hip_index_prepare_nearest_dev / giql_hip_nearest_indexed_dev): the part
that needs no GPU -- the symbols are exported, bound and declared, NULL arguments are refused before a device is
touched, and execute()'s routing predicate.  The results are checked on the GPU (test_index_nearest_gpu.py)."""

import ctypes
import os
import re
from types import SimpleNamespace

from giql_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("giql_hip_index_prepare_nearest_dev", "giql_hip_nearest_indexed_dev")


def test_the_two_symbols_are_exported_bound_and_declared():
    L = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "giql_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(L, name), name
        assert name in _lib.SYMBOLS, name
        assert getattr(L, name).argtypes, name          # bound with argtypes
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert L.giql_hip_abi_version() == 4                # symbols were added, no struct changed


def test_null_arguments_are_invalid_without_a_device():
    L = _lib.load()
    side = _lib.CSide(None, None, None, 0, 0, 0)
    fake = ctypes.create_string_buffer(64)              # stands for a non-NULL handle: it must not be looked into
    h = ctypes.cast(fake, ctypes.c_void_p)
    idx_out = (ctypes.c_int32 * 4)(7, 7, 7, 7)
    dist_out = (ctypes.c_int64 * 4)(7, 7, 7, 7)
    pi, pd = ctypes.cast(idx_out, ctypes.c_void_p), ctypes.cast(dist_out, ctypes.c_void_p)
    for ctx, idx in ((None, None), (None, h), (h, None)):
        assert L.giql_hip_index_prepare_nearest_dev(ctx, idx, None) == _lib.GIQL_ERR_INVALID
        assert b"NULL" in L.giql_hip_last_error()
        assert L.giql_hip_nearest_indexed_dev(ctx, idx, ctypes.byref(side), 0, -1, pi, pd, None) == _lib.GIQL_ERR_INVALID
        assert b"NULL" in L.giql_hip_last_error()
    # NULL outputs: refused before the handles are looked into
    for oi, od in ((None, pd), (pi, None), (None, None)):
        assert L.giql_hip_nearest_indexed_dev(h, h, ctypes.byref(side), 0, -1, oi, od, None) == _lib.GIQL_ERR_INVALID
        assert b"NULL" in L.giql_hip_last_error()
    assert list(idx_out) == [7] * 4 and list(dist_out) == [7] * 4      # nothing was written
    assert bytes(fake.raw) == b"\0" * 64


def test_the_routing_predicate_of_execute():
    from giql_amd import execute as ex

    pin = SimpleNamespace(index=True)
    plan = SimpleNamespace(kind="NEAREST", k=1, stranded=False, residuals=())

    def routed(p=plan, pins=None, devices=None):
        return ex._routes_indexed_nearest(p, {"l": None, "r": pin} if pins is None else pins, devices)

    assert routed() and routed(devices=[0])
    assert not routed(SimpleNamespace(kind="NEAREST", k=2, stranded=False, residuals=()))
    assert not routed(SimpleNamespace(kind="NEAREST", k=1, stranded=True, residuals=()))
    assert not routed(SimpleNamespace(kind="INNER", k=1, stranded=False, residuals=()))
    assert not routed(devices=[0, 1])                                   # one device only
    assert not routed(pins={"l": pin, "r": None})                       # only the left table pinned
    assert not routed(pins={"l": None, "r": SimpleNamespace(index=False)})
    assert set(ex._INDEXED_NEAREST_FORMS) == {"fixed_length", "general"}

    # the index form decides: a stub engine whose index is of the form that is switched off is never called
    class Index:
        general = False

        def prepare_nearest(self):
            raise AssertionError("the switched-off form must not reach the index")

    saved = dict(ex._INDEXED_NEAREST_FORMS)
    real = ex._pinned_index
    try:
        ex._INDEXED_NEAREST_FORMS.update(fixed_length=False, general=True)
        ex._pinned_index = lambda pin_, it, iside, eng: (Index(), ["chr1"])
        assert ex._indexed_nearest(SimpleNamespace(right=None, left=None), None, None, pin, None) is None
        ex._pinned_index = lambda pin_, it, iside, eng: (None, ["chr1"])  # a table without an index
        assert ex._indexed_nearest(SimpleNamespace(right=None, left=None), None, None, pin, None) is None
    finally:
        ex._pinned_index = real
        ex._INDEXED_NEAREST_FORMS.clear()
        ex._INDEXED_NEAREST_FORMS.update(saved)
