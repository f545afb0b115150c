"""The callers of the sort driver launch what they launched, and report the bytes they reported, when
``tests/golden/sort_driver_launches.json`` was recorded -- and answer what the CPU references answer.

What a sort does is decided on the host (``plan_sort`` of giql_amd/csrc/sort_plan.h, carried out by
``run_sort_onesweep``): how many global passes, on which digits, from which buffer into which, whether a bucket stage
follows and which one, and the algorithmic bytes each phase reports.  ``tests/test_row_op_launches_gpu.py`` pins the
per-row operators; this file pins the other callers: the INNER plan and the one-call join (general, fixed-length,
exchanged, presorted and irregular inputs; two, three and four global passes; the fused count and the join in the
bucket stage; the classic sort and another block shape), the index build and the operators that read an index,
CLUSTER / MERGE / DISJOIN and the CONTAINS join.  ``tools/record_sort_driver_launches.py`` holds the calls (one
context per group: a call's path depends on the calls before it) and recorded the fixture at the commit the file
names; it is never regenerated from the code under test."""

import functools
import importlib.util
import json
import os

import numpy as np
import pytest

import _contain_ref as CR
import _disjoin_ref as DJ
from oracle import pyoracle as ora

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("record_sort_driver_launches",
                                               os.path.join(HERE, "..", "tools", "record_sort_driver_launches.py"))
REC = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(REC)


@functools.lru_cache(maxsize=None)
def fixture():
    with open(os.path.join(HERE, "golden", "sort_driver_launches.json")) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_cases_of_the_list():
    doc = fixture()
    ids = [s["id"] for _name, _env, steps in REC.GROUPS for s in steps]
    assert len(ids) == len(set(ids)) and sorted(doc["cases"]) == sorted(ids)
    assert len(doc["recorded_at_commit"]) == 40
    for cid, rec in doc["cases"].items():
        assert set(rec) == {"phase_launches", "phase_bytes", *REC.STAT_KEYS}, cid


# ---------------------------------------------------------------- the CPU references, once per pair of tables
def _side(name):
    return ora.Side(*REC.table(name))


@functools.lru_cache(maxsize=None)
def _inner_pairs(a, b):
    return ora.sort_pairs(*ora.c_inner(_side(a), _side(b), "sweep"))


@functools.lru_cache(maxsize=None)
def _contain_pairs(a, b):
    return CR.contain_pairs(*REC.table(a), *REC.table(b))


def _rows_equal(b, got, exp):
    """The matched rows by their (start, end): ties between equal rows count as equal."""
    ok = exp >= 0
    return (np.array_equal(got >= 0, ok) and np.array_equal(b.start[got[ok]], b.start[exp[ok]])
            and np.array_equal(b.end[got[ok]], b.end[exp[ok]]))


def check(s, out):
    op, cid = s["op"], s["id"]
    if op in ("plan_fill", "join_into", "inner_join_indexed"):
        assert np.array_equal(ora.sort_pairs(*out), _inner_pairs(s["a"], s["b"])), cid
    elif op == "index_create":
        assert out == (), cid
    elif op == "count_indexed":
        assert np.array_equal(out[0], ora.c_count(_side(s["a"]), _side(s["b"]), "sweep")), cid
    elif op == "nearest_indexed":
        wi, wd = ora.c_nearest_k1(_side(s["a"]), _side(s["b"]), method="sweep")
        assert np.array_equal(out[1], wd) and _rows_equal(_side(s["b"]), out[0], wi), cid
    elif op == "cluster":
        assert np.array_equal(out[0], ora.c_cluster(_side(s["b"]), REC.CLUSTER_DISTANCE)), cid
    elif op == "merge":
        want = ora.c_merge(_side(s["b"]), REC.CLUSTER_DISTANCE)
        assert len(out) == len(want) and all(np.array_equal(g, w) for g, w in zip(out, want)), cid
    elif op == "disjoin":
        ref = () if s["a"] is None else REC.table(s["b"])
        target = REC.table(s["b"] if s["a"] is None else s["a"])
        got = np.stack(out, 1).astype(np.int64)
        assert np.array_equal(got, DJ.brute_force_arrays(*target, *ref)), cid
    elif op == "contain_join":
        assert np.array_equal(CR.sort_pairs(np.stack(out, 1)), _contain_pairs(s["a"], s["b"])), cid
    else:
        raise KeyError(op)


def test_the_cases_are_not_trivial():
    """CPU: the tables reach what the case names promise (checked on the references alone)."""
    assert 0 < _inner_pairs("a", "b_mixed").shape[0] and 0 < _inner_pairs("a", "b_fixed").shape[0]
    assert np.array_equal(_inner_pairs("b_fixed", "a"), ora.sort_pairs(*_inner_pairs("a", "b_fixed").T[::-1]))
    for name in ("a_sorted", "b_fixed_sorted"):
        c, s, e = REC.table(name)
        key = c.astype(np.int64) << 32 | s
        assert np.all(np.diff(key) >= 0) and sorted(zip(c, s, e)) == sorted(zip(*REC.table(name[:-7])))
        c, s, _ = REC.table(name[:-7])
        assert np.any(np.diff(c.astype(np.int64) << 32 | s) < 0)            # the original is not sorted
    for name in ("a_zero", "b_zero"):
        assert np.sum(_side(name).end == _side(name).start) >= 20
    assert len(np.unique(_side("b_fixed").end - _side("b_fixed").start)) == 1
    assert 0 < _contain_pairs("a", "b_mixed").shape[0] and 0 < _contain_pairs("a", "b_fixed").shape[0]
    assert len(set(ora.c_cluster(_side("b_mixed"), REC.CLUSTER_DISTANCE).tolist())) > 1


# ---------------------------------------------------------------- the replay
@pytest.mark.parametrize("group", REC.GROUPS, ids=[g[0] for g in REC.GROUPS])
def test_launches_bytes_and_results(group):
    _name, env, steps = group
    recorded = fixture()["cases"]
    for s, out, record in REC.run_group(env, steps):
        print(s["id"], record)
        assert record == recorded[s["id"]], (s["id"], record, recorded[s["id"]])
        check(s, out)
