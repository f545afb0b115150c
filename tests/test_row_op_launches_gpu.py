"""The per-row operators launch what they launched when ``tests/golden/row_op_launches.json`` was recorded, and answer
what the CPU references answer.

The host side of SEMI / ANTI / COUNT, NEAREST, group_rows, their CONTAINS / WITHIN / DISTANCE forms and the
within-distance join is built from shared stages; the order and the number of launches per phase on every path --
first and speculated calls, the missed guess and its repeat, an empty right side, the irregular tails, the three-stage
sort, NEAREST's probe / raw-column keys / two-sort plan, the clamp of a large widening -- is the behaviour a
rearrangement of those stages has to keep.  ``tools/record_row_op_launches.py`` holds the calls (one context per
group: a call's path depends on the calls before it) and recorded the fixture at the commit the file names; it is
never regenerated from the code under test."""

import functools
import importlib.util
import json
import os

import numpy as np
import pytest

import _contain_ref as CR
import _distance_ref as DR
import _rows_ref as RR
from oracle import pyoracle as ora

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("record_row_op_launches",
                                               os.path.join(HERE, "..", "tools", "record_row_op_launches.py"))
REC = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(REC)


@functools.lru_cache(maxsize=None)
def fixture():
    with open(os.path.join(HERE, "golden", "row_op_launches.json")) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_cases_of_the_list():
    doc = fixture()
    ids = [s["id"] for _name, _env, steps in REC.GROUPS for s in steps]
    assert len(ids) == len(set(ids)) and sorted(doc["cases"]) == sorted(ids)
    assert len(doc["recorded_at_commit"]) == 40


# ---------------------------------------------------------------- the CPU references, once per (call, tables)
def _side(name):
    return ora.Side(*REC.table(name))


@functools.lru_cache(maxsize=None)
def _pred_pairs(a, b, predicate, max_distance):
    ta, tb = REC.table(a), REC.table(b)
    if predicate == "contains":
        return CR.contain_pairs(*ta, *tb)
    if predicate == "within":
        return RR.transpose(CR.contain_pairs(*tb, *ta))
    if max_distance < 0:                         # `< 0`: no pair
        return np.zeros((0, 2), np.int64)
    return DR.window_pairs(*ta, *tb, max_distance)


def _rows_equal(b, got, exp):
    """The matched rows by their (start, end): ties between equal rows count as equal."""
    ok = exp >= 0
    return (np.array_equal(got >= 0, ok) and np.array_equal(b.start[got[ok]], b.start[exp[ok]])
            and np.array_equal(b.end[got[ok]], b.end[exp[ok]]))


def check(s, out):
    op, args, cid = s["op"], s["args"], s["id"]
    b = _side(s["b"])
    a = _side(s["a"]) if s["a"] else None
    if op in ("semi", "anti"):
        assert np.array_equal(out[0], ora.c_semi_anti(a, b, op == "anti")), cid
    elif op == "count":
        assert np.array_equal(out[0], ora.c_count(a, b, "sweep")), cid
    elif op in ("nearest", "nearest32"):
        idx, dist = (out[0][:, 0], out[0][:, 1]) if op == "nearest32" else out
        wi, wd = ora.c_nearest_k1(a, b, method="sweep")
        assert np.array_equal(dist, wd) and _rows_equal(b, idx, wi), cid
        if s["a"] == "a_pile":                   # every row of the pile is at one distance: the smallest end wins
            assert np.all(b.end[idx[-5:]] == REC.PILE_START + 4000 - 10 * (REC.PILE_ROWS - 1)), cid
    elif op == "nearest_k":
        wi, wd = ora.c_nearest_k(a, b, args["k"])
        assert np.array_equal(out[1], wd) and _rows_equal(b, out[0], wi), cid
    elif op == "group_rows":
        gid, rep = out
        trip = np.stack([b.chrom, b.start, b.end], 1)
        assert rep.shape[0] == np.unique(trip, axis=0).shape[0] and np.array_equal(trip[rep[gid]], trip), cid
    elif op in ("semi_pred", "count_pred"):
        pairs = _pred_pairs(s["a"], s["b"], args["predicate"], args.get("max_distance"))
        semi, anti, counts = RR.reduce_pairs(pairs, a.n)
        want = counts if op == "count_pred" else (anti if args["anti"] else semi)
        assert np.array_equal(out[0], want), cid
    elif op == "window_join":
        want = DR.window_pairs(*REC.table(s["a"]), *REC.table(s["b"]), args["max_distance"])
        assert np.array_equal(ora.sort_pairs(*out), want), cid
    else:
        raise KeyError(op)


def test_the_cases_are_not_trivial():
    """CPU: the tables reach what the case names promise (checked on the references alone)."""
    a, b = _side("a"), _side("b_mixed")
    assert 0 < ora.c_semi_anti(a, b, False).size < a.n
    for pred, n in (("contains", None), ("within", None), ("within_distance", 0), ("within_distance", 1000)):
        semi, anti, counts = RR.reduce_pairs(_pred_pairs("a_zero", "b_zero", pred, n), a.n)
        assert semi.size > 0 and anti.size > 0, pred
    assert len(np.unique(b.end - b.start)) > 1 and len(np.unique(_side("b_fixed").end - _side("b_fixed").start)) == 1
    for name in ("a_zero", "b_zero"):
        assert np.sum(_side(name).end == _side(name).start) >= 20
    p = _side("b_pile")
    pile = p.start == REC.PILE_START
    assert pile.sum() > 32 and np.all(np.diff(p.end[pile]) < 0)
    assert np.array_equal(_pred_pairs("a_zero", "b_zero", "within_distance", REC.CLAMP_N),
                          _pred_pairs("a_zero", "b_zero", "within_distance", 1 << 40))


# ---------------------------------------------------------------- the replay
@pytest.mark.parametrize("group", REC.GROUPS, ids=[g[0] for g in REC.GROUPS])
def test_launches_and_results(group):
    _name, env, steps = group
    recorded = fixture()["cases"]
    for s, out, record in REC.run_group(env, steps):
        print(s["id"], record)
        assert record == recorded[s["id"]], (s["id"], record, recorded[s["id"]])
        check(s, out)
