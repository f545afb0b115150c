"""The ``range_sets`` opt-in on the CPU: the language (docs/dialect/quantifiers.rst), the plan field, the folds into
residuals, the bounds per table encoding, the errors, the caps -- and the NumPy reference of the GPU tests against
sqlite3's answers (tests/golden/range_sets.json)."""

import json
import os
import re

import numpy as np
import pytest

import _range_set_ref as ref
from giql_amd import _lib, range_sets
from giql_amd.engine import ENCODING_OFFSETS
from giql_amd.plan import JoinPlan, Operand, RangeSet, Residual
from giql_amd.shape import HipDeclined
from giql_amd.table import Table
from giql_amd.transpile import build_plan, transpile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "range_sets.json")

# every example of docs/dialect/quantifiers.rst, comments and layout as printed there: (text, sets the kernel answers,
# residuals).  The three syntax lines stand in the chapter as bare predicates; they are given a SELECT here.
DOCUMENTED = [
    ("SELECT * FROM t WHERE interval INTERSECTS ANY('chr1:1000-2000', 'chr1:5000-6000', 'chr2:1000-3000')", 1, 0),
    ("SELECT * FROM t WHERE interval CONTAINS ANY('chr1:1500', 'chr1:2500')", 1, 0),
    ("SELECT * FROM t WHERE interval WITHIN ANY('chr1:0-10000', 'chr2:0-10000')", 1, 0),
    ("""SELECT * FROM variants
   WHERE interval INTERSECTS ANY(
       'chr1:1000-2000',
       'chr1:5000-6000',
       'chr2:1000-3000'
   )""", 1, 0),
    ("""SELECT * FROM peaks
   WHERE interval INTERSECTS ANY(
       'chr1:11869-12869',   -- Gene A promoter
       'chr1:29554-30554',   -- Gene B promoter
       'chr1:69091-70091'    -- Gene C promoter
   )""", 1, 0),
    ("""SELECT * FROM variants
   WHERE interval INTERSECTS ANY('chr1:1000-2000', 'chr2:5000-6000')
     AND quality >= 30
     AND filter = 'PASS'""", 1, 2),
    ("""SELECT * FROM features
   WHERE interval INTERSECTS ANY(
       'chr1:100000-200000',
       'chr2:100000-200000',
       'chr3:100000-200000',
       'chrX:100000-200000'
   )""", 1, 0),
    ("SELECT * FROM t WHERE interval CONTAINS ALL('chr1:1500', 'chr1:1600', 'chr1:1700')", 0, 3),
    ("SELECT * FROM t WHERE interval INTERSECTS ALL('chr1:1000-1100', 'chr1:1050-1150')", 0, 3),
    ("""SELECT * FROM genes
   WHERE interval CONTAINS ALL(
       'chr1:1500',
       'chr1:1600',
       'chr1:1700'
   )""", 0, 3),
    ("""SELECT * FROM features
   WHERE interval CONTAINS ALL(
       'chr1:10000',
       'chr1:15000',
       'chr1:20000'
   )""", 0, 3),
    ("""SELECT * FROM features
   WHERE interval INTERSECTS ALL(
       'chr1:1000-2000',
       'chr1:1500-2500'
   )

   -- This finds features that overlap BOTH ranges
   -- (i.e., features in the intersection: chr1:1500-2000)""", 0, 3),
    ("""SELECT * FROM peaks
   WHERE NOT interval INTERSECTS ANY(
       'chr1:1000000-2000000',  -- Centromere
       'chr1:5000000-5500000'   -- Known artifact region
   )""", 1, 0),
    ("""SELECT * FROM features
   WHERE interval INTERSECTS ANY('chr1:1000-2000', 'chr1:5000-6000')
     AND interval CONTAINS ALL('chr1:1100', 'chr1:1200')""", 1, 3),
]


@pytest.mark.parametrize("k", range(len(DOCUMENTED)))
def test_every_documented_example_lowers_with_the_opt_in(k):
    text, n_sets, n_residuals = DOCUMENTED[k]
    plan = build_plan(text, None, range_sets=True)
    assert plan.kind == "FILTER" and plan.right is None
    assert len(plan.range_sets) == n_sets and len(plan.residuals) == n_residuals
    assert transpile(text, None, dialect="hip", range_sets=True) == plan.to_string()


@pytest.mark.parametrize("k", range(len(DOCUMENTED)))
def test_without_the_opt_in_the_same_queries_decline_as_before(k):
    text = DOCUMENTED[k][0]
    if "--" in text:        # a comment is no token of the parser without the opt-in
        with pytest.raises(ValueError):
            build_plan(text, None)
        text = re.sub(r"--[^\n]*", "", text)
    with pytest.raises(HipDeclined, match=r"^no join \(a single-table predicate\)"):
        build_plan(text, None)


def test_the_reasons_beside_a_literal_and_inside_a_join_stay():
    for word in ("INTERSECTS", "CONTAINS", "WITHIN"):
        q = f"SELECT * FROM t WHERE interval INTERSECTS 'chr1:1-5' AND interval {word} ANY('chr1:1-2', 'chr1:3-4')"
        with pytest.raises(HipDeclined, match=rf"^{word} ANY/ALL"):
            build_plan(q, None)
        assert len(build_plan(q, None, range_sets=True).range_sets) == 1
        join = f"SELECT a.* FROM a JOIN b ON a.interval INTERSECTS b.interval WHERE a.interval {word} ANY('chr1:1-2', 'chr1:3-4')"
        for opt in (False, True):       # a quantified predicate inside a join is out of scope: the opt-in changes nothing
            with pytest.raises(HipDeclined, match=rf"^{word} ANY/ALL"):
                build_plan(join, None, range_sets=opt)
        lit = f"SELECT a.* FROM a JOIN b ON a.interval INTERSECTS b.interval WHERE a.interval {word} 'chr1:1-2'"
        for opt in (False, True):
            with pytest.raises(HipDeclined, match=rf"^literal-range {word} inside a join"):
                build_plan(lit, None, range_sets=opt)
    with pytest.raises(HipDeclined, match="^NOT over a spatial predicate"):
        build_plan("SELECT * FROM t WHERE NOT interval INTERSECTS 'chr1:1-5'", None)
    with pytest.raises(HipDeclined, match="^more than one spatial predicate"):
        build_plan("SELECT * FROM t WHERE interval INTERSECTS 'chr1:1-5' AND interval CONTAINS 'chr1:2'", None)
    with pytest.raises(HipDeclined, match="^literal range formats other than"):
        build_plan("SELECT * FROM t WHERE interval INTERSECTS 'chr1:[1,5)'", None)
    with pytest.raises(HipDeclined, match="^literal predicate over a non-canonical table"):
        build_plan("SELECT * FROM t WHERE interval INTERSECTS 'chr1:1-5'", [Table("t", coordinate_system="1based")])
    with pytest.raises(HipDeclined, match="^spatial predicate under OR"):
        build_plan("SELECT * FROM t WHERE interval INTERSECTS ANY('chr1:1-5', 'chr1:7-9') OR score > 1", None, range_sets=True)
    for tail in ("GROUP BY chrom", "ORDER BY start"):
        with pytest.raises(HipDeclined):
            build_plan(f"SELECT * FROM t WHERE interval INTERSECTS ANY('chr1:1-5', 'chr1:7-9') {tail}", None, range_sets=True)
    with pytest.raises(HipDeclined, match="^DISTINCT over a literal-range filter"):
        build_plan("SELECT DISTINCT chrom FROM t WHERE interval INTERSECTS ANY('chr1:1-5', 'chr1:7-9')", None, range_sets=True)


def test_some_is_any_and_sets_are_canonical_triples():
    any_ = build_plan("SELECT * FROM t WHERE interval WITHIN ANY('chr1:[10,20]', 'chr2:7', 'chr1:5-9:-')", None, range_sets=True)
    some = build_plan("SELECT * FROM t WHERE interval WITHIN SOME('chr1:[10,20]', 'chr2:7', 'chr1:5-9:-')", None, range_sets=True)
    assert any_ == some
    assert any_.range_sets == (RangeSet("within", "any", False, (("chr1", 10, 21), ("chr2", 7, 8), ("chr1", 5, 9))),)
    dup = build_plan("SELECT * FROM t WHERE NOT interval CONTAINS ANY('chr1:5', 'chr1:[5,6)', 'chr1:9')", None, range_sets=True)
    assert dup.range_sets == (RangeSet("contains", "any", True, (("chr1", 5, 6), ("chr1", 9, 10))),)


def test_plan_strings_round_trip_and_old_strings_load_without_the_field():
    q = ("SELECT chrom, start AS s FROM t WHERE interval INTERSECTS ANY('chr1:1-5', 'chrX:[7,9]') "
         "AND NOT interval WITHIN SOME('chr2:1-50', 'chr2:40-90') AND interval CONTAINS ALL('chr1:2', 'chr1:3') AND score > 3")
    plan = build_plan(q, [Table("t", coordinate_system="1based", interval_type="closed")], range_sets=True)
    assert [(r.op, r.negated) for r in plan.range_sets] == [("intersects", False), ("within", True)]
    text = plan.to_string()
    assert JoinPlan.from_string(text) == plan and JoinPlan.from_string(text).to_string() == text
    assert JoinPlan.from_dict(json.loads(json.dumps(plan.to_dict()))) == plan
    old = build_plan("SELECT * FROM t WHERE interval INTERSECTS 'chr1:1-5'", None)
    d = old.to_dict()
    assert d.pop("range_sets") == []
    assert JoinPlan.from_dict(d) == old and JoinPlan.from_dict(d).range_sets == ()
    with pytest.raises(ValueError, match="need a FILTER plan"):
        JoinPlan("SEMI", old.left, old.left, range_sets=plan.range_sets)


def _res(col, op, value, group=0):
    return Residual("where", Operand("l", col), op, Operand("str" if isinstance(value, str) else "int", value), group)


def test_a_single_literal_lowers_as_it_does_without_the_opt_in():
    for q in ("SELECT * FROM t WHERE interval INTERSECTS 'chr1:1000-2000' AND score > 3",
              "SELECT name FROM t WHERE interval CONTAINS 'chr1:150-250'", "SELECT * FROM t x WHERE x.interval WITHIN 'chr2:5-9'"):
        assert build_plan(q, None, range_sets=True) == build_plan(q, None)
    one = build_plan("SELECT * FROM t WHERE interval INTERSECTS ANY('chr1:1000-2000')", None, range_sets=True)
    assert one == build_plan("SELECT * FROM t WHERE interval INTERSECTS 'chr1:1000-2000'", None)


def test_the_folds():
    # a single point literal: CONTAINS in its point form, end > 150, is end >= 151 on integers
    point = build_plan("SELECT * FROM t WHERE interval CONTAINS 'chr1:150'", None, range_sets=True)
    assert point.residuals == (_res("chrom", "=", "chr1"), _res("start", "<=", 150), _res("end", ">=", 151))
    assert not point.range_sets
    # ALL across two chromosomes: one equality per chromosome (never both true: exactly the reference's AND), the
    # tightest bound of each column
    two = build_plan("SELECT * FROM t WHERE interval INTERSECTS ALL('chr1:100-200', 'chr2:150-300', 'chr1:120-180')", None,
                     range_sets=True)
    assert two.residuals == (_res("chrom", "=", "chr1"), _res("chrom", "=", "chr2"), _res("start", "<", 180),
                             _res("end", ">", 150))
    within = build_plan("SELECT * FROM t WHERE interval WITHIN ALL('chr1:100-900', 'chr1:50-700')", None, range_sets=True)
    assert within.residuals == (_res("chrom", "=", "chr1"), _res("start", ">=", 100), _res("end", "<=", 700))
    # NOT ALL: one OR-group of the negated comparisons
    neg = build_plan("SELECT * FROM t WHERE NOT interval CONTAINS ALL('chr1:150', 'chr1:300') AND score > 1", None,
                     range_sets=True)
    assert neg.residuals[0] == _res("score", ">", 1)
    groups = {r.group for r in neg.residuals[1:]}
    assert len(groups) == 1 and 0 not in groups
    g = groups.pop()
    assert neg.residuals[1:] == (_res("chrom", "!=", "chr1", g), _res("start", ">", 150, g), _res("end", "<", 301, g))
    # NOT over a single literal, beside an OR-group of the query's own: two different groups
    both = build_plan("SELECT * FROM t WHERE (score > 1 OR score < -1) AND NOT interval INTERSECTS 'chr1:5-9'", None,
                      range_sets=True)
    assert [r.group for r in both.residuals] == [1, 1, 2, 2, 2]
    assert both.residuals[2:] == (_res("chrom", "!=", "chr1", 2), _res("start", ">=", 9, 2), _res("end", "<=", 5, 2))
    # NOT NOT is no NOT
    assert build_plan("SELECT * FROM t WHERE NOT (NOT interval INTERSECTS 'chr1:5-9')", None, range_sets=True).residuals == \
        build_plan("SELECT * FROM t WHERE interval INTERSECTS 'chr1:5-9'", None).residuals


@pytest.mark.parametrize("encoding", list(ENCODING_OFFSETS))
def test_the_bounds_move_onto_the_literal_for_every_encoding(encoding):
    so, eo = ENCODING_OFFSETS[encoding]
    assert range_sets.CANONICAL_OFFSETS[encoding] == (so, eo)
    table = [Table("t", coordinate_system=encoding[0], interval_type=encoding[1])]
    r = ("chr1", 1000, 2000)
    # start + so < 2000 AND end + eo > 1000, and so on: the column stays bare
    assert range_sets.bounds("intersects", r, encoding) == (2000 - so, 1000 - eo)
    assert range_sets.bounds("contains", r, encoding) == (1000 - so, 2000 - eo)
    assert range_sets.bounds("within", r, encoding) == (1000 - so, 2000 - eo)
    plan = build_plan("SELECT * FROM t WHERE interval INTERSECTS 'chr1:1000-2000' AND NOT interval WITHIN 'chr1:[1000,1999]'",
                      table, range_sets=True)
    assert plan.residuals[:3] == (_res("chrom", "=", "chr1"), _res("start", "<", 2000 - so), _res("end", ">", 1000 - eo))
    assert plan.residuals[3:] == (_res("chrom", "!=", "chr1", 1), _res("start", "<", 1000 - so, 1), _res("end", ">", 2000 - eo, 1))
    # every raw row of the encoding compares as its canonical form does, at the edges of the range
    for raw_s, raw_e in ((999 - so, 1000 - eo), (999 - so, 1001 - eo), (2000 - so, 2001 - eo), (1999 - so, 2005 - eo)):
        bs, be = range_sets.bounds("intersects", r, encoding)
        assert (raw_s < bs and raw_e > be) == (raw_s + so < 2000 and raw_e + eo > 1000)
    # beyond int64 a bound saturates: no int32 (or int64) value compares differently
    big = range_sets.bounds("within", ("chr1", 0, 10**30), encoding)
    assert big[1] == 2**63 - 1 and -2**63 <= big[0] <= 1


def test_the_five_formats_and_the_errors():
    assert range_sets.parse_range("chr1:1000-2000") == ("chr1", 1000, 2000)
    assert range_sets.parse_range("chr1:[1000,2000)") == ("chr1", 1000, 2000)
    assert range_sets.parse_range("chr1:[1001,2000]") == ("chr1", 1001, 2001)
    assert range_sets.parse_range("chr1:1500") == ("chr1", 1500, 1501)
    assert range_sets.parse_range("chr1:1000-2000:+") == ("chr1", 1000, 2000)
    assert range_sets.parse_range("chr1:[1000,2000):-") == ("chr1", 1000, 2000)
    assert range_sets.parse_range("chr1:[1000,2000]:-") == ("chr1", 1000, 2001)
    assert range_sets.parse_range(" chr1.1_x:5-6 ") == ("chr1.1_x", 5, 6)
    for bad in ("chr1", "chr1:", "chr1:a-b", "chr1:5-", "chr1:(5,6)", "chr1:5:+", "chr1:5-6:*", "chr 1:5-6", ""):
        with pytest.raises(ValueError, match="^Could not parse genomic range") as exc:
            build_plan(f"SELECT * FROM t WHERE interval INTERSECTS ANY('chr1:1-2', '{bad}')", None, range_sets=True)
        assert not isinstance(exc.value, HipDeclined)
        with pytest.raises(ValueError, match="^Could not parse genomic range"):
            build_plan(f"SELECT * FROM t WHERE NOT interval WITHIN '{bad}'", None, range_sets=True)
    for inverted in ("chr1:20-10", "chr1:5-5", "chr1:[5,5)", "chr1:[5,5]", "chr1:[9,3]:+"):
        with pytest.raises(ValueError, match="^Start must be less than end") as exc:
            build_plan(f"SELECT * FROM t WHERE interval CONTAINS ALL('chr1:1', '{inverted}')", None, range_sets=True)
        assert not isinstance(exc.value, HipDeclined)
    with pytest.raises(ValueError, match="is not the genomic column"):
        build_plan("SELECT * FROM t WHERE score INTERSECTS ANY('chr1:1-2', 'chr1:3-4')", None, range_sets=True)


def test_the_caps_decline_with_reasons_of_their_own():
    def any_of(k, chrom="chr1"):
        return "interval INTERSECTS ANY(" + ", ".join(f"'{chrom}:{10 * i}-{10 * i + 5}'" for i in range(k)) + ")"

    assert len(build_plan(f"SELECT * FROM t WHERE {any_of(1024)}", None, range_sets=True).range_sets[0].ranges) == 1024
    with pytest.raises(HipDeclined, match="^more than 1024 ranges in one ANY"):
        build_plan(f"SELECT * FROM t WHERE {any_of(1025)}", None, range_sets=True)
    eight = " AND ".join(any_of(2, f"chr{i}") for i in range(8))
    assert len(build_plan(f"SELECT * FROM t WHERE {eight}", None, range_sets=True).range_sets) == 8
    with pytest.raises(HipDeclined, match="^more than 8 ANY"):
        build_plan(f"SELECT * FROM t WHERE {eight} AND {any_of(2, 'chr9')}", None, range_sets=True)
    # ALL folds to three comparisons however many ranges it names; six of them are 18 predicates
    all_of = "interval CONTAINS ALL(" + ", ".join(f"'chr1:{i}'" for i in range(2000)) + ")"
    assert len(build_plan(f"SELECT * FROM t WHERE {all_of}", None, range_sets=True).residuals) == 3
    with pytest.raises(HipDeclined, match="^a range-set filter that needs more than 16 predicates"):
        build_plan("SELECT * FROM t WHERE " + " AND ".join(["interval CONTAINS ALL('chr1:5', 'chr1:6')"] * 6), None, range_sets=True)
    assert (range_sets.MAX_KERNEL_SETS, range_sets.MAX_SET_RANGES) == (_lib.RANGE_MAX_SETS, _lib.RANGE_MAX_RANGES)


def test_the_abi_declares_the_entry_point():
    header = open(os.path.join(ROOT, "include", "giql_hip_range_sets.h")).read()
    assert "int giql_hip_range_set_any_dev(giql_hip_ctx* ctx, const int32_t* chrom" in header
    declared = sorted(set(re.findall(r"\b(giql_hip_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))))
    assert declared == sorted(_lib.RANGE_SET_SYMBOLS)
    for name, value in (("GIQL_RANGE_INTERSECTS", 0), ("GIQL_RANGE_CONTAINS", 1), ("GIQL_RANGE_WITHIN", 2),
                        ("GIQL_RANGE_MAX_SETS", 8), ("GIQL_RANGE_MAX_RANGES", 1024)):
        assert re.search(rf"#define {name}\s+{value}\b", header), name
    assert _lib.RANGE_OPS == {"intersects": 0, "contains": 1, "within": 2}
    L = _lib.load()
    assert all(hasattr(L, name) for name in _lib.RANGE_SET_SYMBOLS)
    assert len(L.giql_hip_range_set_any_dev.argtypes) == 11
    import ctypes

    assert ctypes.sizeof(_lib.CRangeSet) == 48 and _lib.CRangeSet.out_valid.offset == 40
    _struct_matches_the_header()
    # refused before any device is touched
    assert L.giql_hip_range_set_any_dev(None, None, None, None, None, None, None, 0, None, 0, None) == _lib.GIQL_ERR_INVALID


def _struct_matches_the_header():
    """The ctypes mirror against the REAL C layout: a probe compiled from the header prints sizeof / offsetof."""
    import shutil
    import subprocess
    import tempfile

    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    fields = ["op", "n_ranges", "chrom", "on_start", "on_end", "out_value", "out_valid"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.join(ROOT, "include", "giql_hip_range_sets.h")}"',
             "int main(void) {", '  printf("size %zu\\n", sizeof(giql_range_set));']
    lines += [f'  printf("{f} %zu\\n", offsetof(giql_range_set, {f}));' for f in fields]
    lines += ["  return 0;", "}"]
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "probe.c"), os.path.join(tmp, "probe")
        open(src, "w").write("\n".join(lines))
        subprocess.run([gcc, "-o", exe, src], check=True)
        got = dict(line.split() for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    import ctypes

    assert ctypes.sizeof(_lib.CRangeSet) == int(got["size"])
    for f in fields:
        assert getattr(_lib.CRangeSet, f).offset == int(got[f]), f


# ------------------------------------------------------------------------- the NumPy reference against sqlite3
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_goldens_conditions_hold():
    g = _golden()
    t = g["tallies"]
    assert t["cases"] == len(g["cases"]) >= 60 and t["largest table"] < 300
    assert 10 * t["first predicate keeps nothing"] <= t["cases"] and 10 * t["first predicate keeps everything"] <= t["cases"]
    assert 2 * t["ANY cases with a row only the aggregate finds"] >= t["ANY cases"] >= 12
    tags = {tag for c in g["cases"] for tag in c["tags"]}
    assert {"intersects", "contains", "within", "any", "all", "not", "nulls", "any-single", "table-only-chrom",
            "ranges-only-chrom", "mixed", "known"} <= tags
    assert {"-".join(e) for e in ENCODING_OFFSETS} <= tags
    assert os.path.getsize(GOLDEN) < 512 * 1024


def test_the_numpy_reference_gives_sqlites_answers():
    for case in _golden()["cases"]:
        assert ref.kept_rows(case) == case["expected"], case["name"]


def test_the_lowered_plan_of_every_golden_case_says_what_the_case_says():
    for case in _golden()["cases"]:
        table = [Table("t", coordinate_system=case["encoding"][0], interval_type=case["encoding"][1])]
        plan = build_plan("SELECT * FROM t WHERE " + case["where"], table, range_sets=True)
        want = [(p["op"], p["negated"], sorted(set(map(tuple, p["ranges"])))) for p in case["predicates"]
                if p["quantifier"] == "any" and len(set(map(tuple, p["ranges"]))) > 1]
        assert [(r.op, r.negated, sorted(r.ranges)) for r in plan.range_sets] == want, case["name"]


def test_any_over_bounds_is_three_valued():
    # chrom 0 named, chrom 1 not: a NULL start is FALSE off the named chromosome and NULL on it; a NULL chrom is
    # FALSE when a known field already fails every range
    chrom = np.array([0, 1, 0, 0, 0], np.int32)
    start = np.array([0, 0, 15, 500, 12], np.int32)
    end = np.array([30, 30, 18, 600, 14], np.int32)
    ok_c = np.array([1, 1, 1, 0, 0], bool)
    ok_s = np.array([0, 0, 1, 1, 1], bool)
    ok_e = np.ones(5, bool)
    value, valid = ref.any_over_bounds("intersects", chrom, start, end, ok_c, ok_s, ok_e, [0, 0], [20, 40], [10, 30])
    assert value.tolist() == [0, 0, 1, 0, 0] and valid.tolist() == [0, 1, 1, 1, 0]
