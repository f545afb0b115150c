"""STRING_AGG beside MERGE (``string_aggregates=True``): the plan builder, the declines, the caps, the C ABI's
declaration and struct layout, the plain-Python restatement against the sqlite-minted rows, and the wide-genome
concatenation of string results on CPU tensors.  The GPU half is tests/test_string_agg_gpu.py."""
import collections
import ctypes
import json
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import _string_agg_ref as S
from giql_amd import _lib
from giql_amd.plan import Aggregate, JoinPlan, Projection
from giql_amd.transpile import HipDeclined, build_plan, transpile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = json.load(open(os.path.join(HERE, "golden", "merge_string_agg.json"), encoding="utf-8"))

# docs/recipes/clustering.rst "Collect Feature Names"
RECIPE = """SELECT
       MERGE(interval),
       STRING_AGG(name, ',') AS merged_features
   FROM features"""


def test_the_recipe_lowers_and_its_plan_string_carries_the_separator():
    plan = build_plan(RECIPE, ["features"], string_aggregates=True)
    assert plan.kind == "MERGE" and plan.distance == 0
    assert plan.projection == (Projection("agg", "0", "merged_features"),)
    assert plan.aggregates == (Aggregate("STRING_AGG", "l", "name", "merged_features", separator=","),)
    text = transpile(RECIPE, ["features"], dialect="hip", string_aggregates=True)
    assert text == plan.to_string() and JoinPlan.from_string(text) == plan
    assert JoinPlan.from_string(text).to_string() == text
    assert json.loads(text[text.index("{"):])["aggregates"][0]["separator"] == ","
    assert JoinPlan.from_dict(json.loads(json.dumps(plan.to_dict()))) == plan


def test_separators_of_every_kind_survive_the_plan_string():
    for sep in ("", ";", "', '", " | ", "→", "\t", "x" * 255, "é" * 127):
        lit = sep.replace("'", "''")
        plan = build_plan(f"SELECT MERGE(interval, 5), STRING_AGG(f.name, '{lit}') AS names FROM features f",
                          ["features"], string_aggregates=True)
        assert plan.aggregates[0].separator == sep
        assert JoinPlan.from_string(plan.to_string()) == plan


def test_without_the_keyword_it_declines_as_before():
    with pytest.raises(HipDeclined, match="function call in the SELECT list"):
        build_plan(RECIPE, ["features"])
    with pytest.raises(HipDeclined):
        transpile(RECIPE, ["features"], dialect="hip")
    with pytest.raises(HipDeclined, match=r"STRING_AGG beside MERGE \(-o collapse\)"):
        build_plan(RECIPE, ["features"], merge_aggregates=True)
    # the keyword alone does not bring the numeric aggregates
    with pytest.raises(HipDeclined, match="function call in the SELECT list"):
        build_plan("SELECT MERGE(interval), SUM(score) AS s FROM features", ["features"], string_aggregates=True)


def test_an_older_plan_string_loads_and_a_numeric_aggregate_serialises_null():
    plan = build_plan("SELECT MERGE(interval), SUM(score) AS s FROM features", ["features"], merge_aggregates=True)
    d = plan.to_dict()
    assert d["aggregates"][0]["separator"] is None and '"separator":null' in plan.to_string()
    del d["aggregates"][0]["separator"]          # what a plan string written before the field existed holds
    assert JoinPlan.from_dict(d) == plan
    with pytest.raises(ValueError, match="carries a separator"):
        JoinPlan("MERGE", plan.left, None, (), aggregates=(Aggregate("SUM", "l", "score", "s", separator=","),))
    with pytest.raises(ValueError, match="carries a separator"):
        JoinPlan("MERGE", plan.left, None, (), aggregates=(Aggregate("STRING_AGG", "l", "name", "s"),))


@pytest.mark.parametrize("query, message", [
    ("SELECT MERGE(interval), STRING_AGG(name) AS names FROM features", "one argument"),
    ("SELECT MERGE(interval), STRING_AGG(name, sep) AS names FROM features", "not a string literal"),
    ("SELECT MERGE(interval), STRING_AGG(name, 7) AS names FROM features", "not a string literal"),
    ("SELECT MERGE(interval), STRING_AGG(name, ',' || ' ') AS names FROM features", "not a string literal"),
    ("SELECT MERGE(interval), STRING_AGG(name, '" + "x" * 256 + "') AS names FROM features", "longer than 255 UTF-8 bytes"),
    ("SELECT MERGE(interval), STRING_AGG(name, '" + "é" * 128 + "') AS names FROM features", "longer than 255 UTF-8 bytes"),
    ("SELECT MERGE(interval), STRING_AGG(DISTINCT name, ',') AS names FROM features", "DISTINCT inside STRING_AGG"),
    ("SELECT MERGE(interval), STRING_AGG(name, ',' ORDER BY name) AS names FROM features", "ORDER BY inside STRING_AGG"),
    ("SELECT MERGE(interval), STRING_AGG(name ORDER BY name) AS names FROM features", "ORDER BY inside STRING_AGG"),
    ("SELECT MERGE(interval), STRING_AGG(name, ',') FROM features", "without an alias beside MERGE"),
    ("SELECT MERGE(interval), STRING_AGG(UPPER(name), ',') AS names FROM features", "expression argument of STRING_AGG"),
    ("SELECT *, CLUSTER(interval) AS cid, STRING_AGG(name, ',') AS names FROM features", "STRING_AGG beside CLUSTER"),
    ("SELECT MERGE(interval), GROUP_CONCAT(name, ',') AS names FROM features", "function call in the SELECT list"),
    ("SELECT MERGE(interval), LISTAGG(name, ',') AS names FROM features", "function call in the SELECT list"),
])
def test_what_declines_says_why(query, message):
    with pytest.raises(HipDeclined, match=message):
        build_plan(query, ["features"], string_aggregates=True, merge_aggregates=True)


def test_mixed_projections_keep_their_order_and_share_the_aggregates():
    q = ("SELECT MERGE(interval, stranded := true), SUM(score) AS total, STRING_AGG(name, ';') AS names, COUNT(*) AS n, "
         "STRING_AGG(name, '') AS glued, MAX(score) AS hi FROM features")
    plan = build_plan(q, ["features"], merge_aggregates=True, string_aggregates=True)
    assert plan.projection == (Projection("agg", "0", "total"), Projection("agg", "1", "names"),
                               Projection("count", "*", "n"), Projection("agg", "2", "glued"), Projection("agg", "3", "hi"))
    assert [(a.func, a.column, a.separator) for a in plan.aggregates] == [
        ("SUM", "score", None), ("STRING_AGG", "name", ";"), ("STRING_AGG", "name", ""), ("MAX", "score", None)]
    assert JoinPlan.from_string(plan.to_string()) == plan


def test_the_caps_eight_in_all_four_strings():
    def q(n_str, n_num):
        items = [f"STRING_AGG(name, '{k}') AS s{k}" for k in range(n_str)] + [f"SUM(c{k}) AS n{k}" for k in range(n_num)]
        return "SELECT MERGE(interval), " + ", ".join(items) + " FROM features"

    both = dict(merge_aggregates=True, string_aggregates=True)
    assert len(build_plan(q(4, 4), ["features"], **both).aggregates) == 8
    assert len(build_plan(q(4, 0), ["features"], string_aggregates=True).aggregates) == 4
    with pytest.raises(HipDeclined, match="more than 4 STRING_AGG"):
        build_plan(q(5, 0), ["features"], **both)
    with pytest.raises(HipDeclined, match="more than 8 aggregates"):
        build_plan(q(4, 5), ["features"], **both)
    with pytest.raises(HipDeclined, match="more than 8 aggregates"):
        build_plan(q(1, 8), ["features"], **both)


def test_the_header_s_symbols_are_the_binding_s():
    header = open(os.path.join(ROOT, "include", "giql_hip_string_agg.h")).read()
    declared = sorted(set(re.findall(r"\b(giql_hip_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))))
    assert declared == sorted(_lib.STRING_AGG_SYMBOLS)
    assert not set(_lib.STRING_AGG_SYMBOLS) & set(_lib.SYMBOLS)
    for name, value in (("GIQL_STR_AGG_MAX", "4"), ("GIQL_STR_AGG_MAX_SEP", "255"), ("GIQL_STR_AGG_NULL_ROW", "0xFFFFFFFFu")):
        assert re.search(rf"#define {name}\s+{value}\b", header), name
    assert (_lib.STR_AGG_MAX, _lib.STR_AGG_MAX_SEP, _lib.STR_AGG_NULL_ROW) == (4, 255, 0xFFFFFFFF)
    main = open(os.path.join(ROOT, "include", "giql_hip.h")).read()
    assert "#define GIQL_HIP_ABI_VERSION 4 " in main and "giql_hip_merge_str_dev" not in main
    L = _lib.load()
    assert L.giql_hip_abi_version() == 4
    assert all(hasattr(L, name) for name in _lib.STRING_AGG_SYMBOLS)
    assert len(L.giql_hip_merge_str_dev.argtypes) == 18 and len(L.giql_hip_concat_utf8_fill_dev.argtypes) == 11
    # refused before any device is touched
    assert L.giql_hip_merge_str_dev(None, None, 0, 0, None, 0, None, 0, None, 0, None, None, None, None, None, 0, None,
                                    None) == _lib.GIQL_ERR_INVALID
    assert L.giql_hip_concat_utf8_fill_dev(None, None, None, 0, None, None, 0, None, 0, None, None) == _lib.GIQL_ERR_INVALID


def test_the_struct_mirror_matches_the_compiled_layout():
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    fields = [f[0] for f in _lib.CStrAgg._fields_]
    assert fields == ["offsets", "valid", "sep_len", "out_offsets", "out_nn", "row_dst", "n_bytes"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.join(ROOT, "include", "giql_hip_string_agg.h")}"',
             "int main(void) {", '  printf("size %zu\\n", sizeof(giql_str_agg));']
    lines += [f'  printf("{f} %zu\\n", offsetof(giql_str_agg, {f}));' for f in fields]
    lines += ["  return 0;", "}"]
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "probe.c"), os.path.join(tmp, "probe")
        open(src, "w").write("\n".join(lines))
        subprocess.run([gcc, "-o", exe, src], check=True)
        got = dict(line.split() for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert ctypes.sizeof(_lib.CStrAgg) == int(got["size"])
    for f in fields:
        assert getattr(_lib.CStrAgg, f).offset == int(got[f]), f


# ------------------------------------------------------------------ the restatement against sqlite's group_concat
def test_the_restatement_s_null_and_empty_string_rules():
    assert S.string_agg([None, None], ",") is None and S.string_agg([], ",") is None
    assert S.string_agg(["", None], ",") == "" and S.string_agg(["", ""], ",") == ","
    assert S.string_agg([None, "a", None, "", "b"], "--") == "a----b"
    assert S.string_agg(["a", "b"], "") == "ab"
    assert S.members_in_order([2, 1, 3, 0], [5, 9, 5, 1]) == [3, 0, 2, 1]   # start, then row


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=lambda c: c["name"])
def test_the_restatement_matches_the_sqlite_minted_rows_as_token_multisets(case):
    rows, sep = GOLDEN["rows"], GOLDEN["separator"]
    part = [(r[0], r[3]) if case["stranded"] else (r[0],) for r in rows]
    got = S.merge_string_agg(part, [r[1] for r in rows], [r[2] for r in rows], case["distance"],
                             {"name": [r[4] for r in rows]}, [("name", sep)])
    k = len(part[0])

    def tokens(s):
        return None if s is None else sorted(collections.Counter(s.split(sep)).items())

    got = sorted(([*r[0], r[1], r[2], r[3], tokens(r[4])] for r in got), key=lambda r: (r[0], r[k]))
    want = sorted(([*r[:k], r[k], r[k + 1], r[k + 2], tokens(r[k + 4])] for r in case["merged"]), key=lambda r: (r[0], r[k]))
    assert got == want
    # the non-NULL count sqlite reports is the number of tokens
    for r in case["merged"]:
        assert r[k + 3] == (0 if r[k + 4] is None else len(r[k + 4].split(sep)))


# ------------------------------------------------------------------ wide.py: string results of several groups
def _utf8(strings):
    import torch

    blob = [s.encode("utf-8") for s in strings]
    off = [0]
    for b in blob:
        off.append(off[-1] + len(b))
    return (torch.tensor(off, dtype=torch.int32),
            torch.tensor(list(b"".join(blob)), dtype=torch.uint8))


def _strings(offsets, data):
    raw = bytes(data.tolist())
    off = offsets.tolist()
    return [raw[off[i]:off[i + 1]].decode("utf-8") for i in range(len(off) - 1)]


def test_wide_concatenates_string_results_in_region_order():
    torch = pytest.importorskip("torch")
    from giql_amd import wide

    groups = [["b1", "", "λλ"], [], ["a0", "x" * 70], ["zz"]]
    cols = [_utf8(g) for g in groups]
    flat = [s for g in groups for s in g]
    order = torch.tensor([3, 0, 5, 1, 4, 2])
    off, data = wide.utf8_in_order(cols, order, torch.device("cpu"))
    assert off.dtype == torch.int32 and data.dtype == torch.uint8 and int(off[0]) == 0
    assert _strings(off, data) == [flat[i] for i in order.tolist()]
    off, data = wide.utf8_in_order([], torch.empty(0, dtype=torch.long), torch.device("cpu"))
    assert off.tolist() == [0] and data.numel() == 0


def test_wide_merge_agg_puts_numeric_and_string_columns_in_one_order():
    torch = pytest.importorskip("torch")
    from giql_amd import wide

    def part(chrom, starts, names, valid, sums):
        n = len(starts)
        i32 = lambda v: torch.tensor(v, dtype=torch.int32)
        return (torch.arange(n), None, (i32([chrom] * n), i32(starts), i32([s + 5 for s in starts]),
                                        torch.ones(n, dtype=torch.int64), _utf8(names) + (torch.tensor(valid),),
                                        (torch.tensor(sums, dtype=torch.int64), torch.ones(n, dtype=torch.bool))))

    # group order is not chromosome order: (chrom 2), then (chrom 0 and 1)
    parts = [part(2, [10, 40], ["c10", ""], [True, False], [1, 2]),
             (torch.arange(3), None, (torch.tensor([0, 1, 0], dtype=torch.int32), torch.tensor([7, 3, 90], dtype=torch.int32),
                                      torch.tensor([9, 5, 95], dtype=torch.int32), torch.ones(3, dtype=torch.int64),
                                      _utf8(["a7", "b3", "a90,x"]) + (torch.tensor([True, True, True]),),
                                      (torch.tensor([3, 4, 5], dtype=torch.int64), torch.ones(3, dtype=torch.bool))))]
    out = wide.merge_agg(parts, torch.device("cpu"), [wide.UTF8, torch.int64])
    assert out[0].tolist() == [0, 0, 1, 2, 2] and out[1].tolist() == [7, 90, 3, 10, 40]
    off, data, valid = out[4]
    assert _strings(off, data) == ["a7", "a90,x", "b3", "c10", ""] and valid.tolist() == [True, True, True, True, False]
    assert out[5][0].tolist() == [3, 5, 4, 1, 2]
    none = wide.merge_agg([], torch.device("cpu"), [wide.UTF8])
    assert none[4][0].tolist() == [0] and none[4][1].numel() == 0 and none[4][2].numel() == 0
