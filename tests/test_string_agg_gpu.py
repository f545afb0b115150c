"""STRING_AGG beside MERGE on the GPU: ``HipEngine.merge_agg`` with string entries and ``execute(...,
string_aggregates=True)`` against tests/_string_agg_ref.py -- exact bytes, members in (start, row) order -- and the
sqlite-minted rows of tests/golden/merge_string_agg.json (token multisets: sqlite's order is its own); then the two C
entry points through ctypes: guarded outputs, argument errors, the plan-lifetime cells."""
import collections
import ctypes
import json
import os

import numpy as np
import pytest

import _merge_agg_ref as R
import _string_agg_ref as S

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "merge_string_agg.json"), encoding="utf-8"))
NT = 256          # SAGG_NT (giql_amd/csrc/string_agg_kernels.hip.h): sorted positions per block
SCAN = 4096       # SCAN_TILE (giql_amd/csrc/scan.hip.h): inputs per block of the three scans
LENGTHS = [0, 1, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000]
SEPARATORS = [b"", b",", b", ", b"abc", b"|--|", b"12345", b"0123456789abcdef", b"0123456789abcdefg", "→".encode(),
              b"s" * 255]
AA = 0xAA


def _engine(env=None):
    from giql_amd.engine import HipEngine

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    with pytest.MonkeyPatch.context() as mp:
        for k, v in (env or {}).items():
            mp.setenv(k, v)
        return HipEngine(0)


@pytest.fixture(scope="module")
def eng():
    e = _engine()
    yield e
    e.close()


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _side(chrom, start, end):
    from giql_amd.engine import DeviceSide

    return DeviceSide.from_numpy(np.asarray(chrom).astype(np.int32), np.asarray(start).astype(np.int32),
                                 np.asarray(end).astype(np.int32), device="cuda:0")


def _utf8(values):
    """A list of ``bytes | None`` as ``(offsets, data, valid | None)`` device tensors (a NULL row holds no bytes)."""
    lens = np.array([0 if v is None else len(v) for v in values], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    data = np.frombuffer(b"".join(v or b"" for v in values), np.uint8).copy()
    valid = None if all(v is not None for v in values) else _dev(np.array([v is not None for v in values], np.uint8))
    return _dev(off), _dev(data), valid


def _decode(offsets, data, valid):
    off, raw, ok = offsets.cpu().tolist(), data.cpu().numpy().tobytes(), valid.cpu().tolist()
    assert off[0] == 0 and off[-1] == len(raw) and len(off) == len(ok) + 1
    assert all(off[g + 1] == off[g] for g in range(len(ok)) if not ok[g])      # a NULL region holds no bytes
    return [raw[off[g]:off[g + 1]] if ok[g] else None for g in range(len(ok))]


def _word(r, length, row):
    """``length`` bytes that name their row: a misplaced or torn value cannot pass for another."""
    tag = b"%d:" % row
    body = bytes(r.integers(97, 123, max(length - len(tag), 0), dtype=np.uint8))
    return (tag + body)[:length]


def _values(r, n, lengths=(0, 1, 3, 5, 8, 12), nulls=0.3):
    return [None if r.random() < nulls else _word(r, int(r.choice(lengths)), i) for i in range(n)]


def run_and_check(eng, chrom, start, end, n_chrom, distance, cols, aggs, preds=None, holds=None, numeric=()):
    """``eng.merge_agg`` with the string entries ``aggs = [(column, separator)]`` (and ``numeric`` entries in front)
    against the restatement, byte for byte.  ``cols``: name -> list of ``bytes | None``.  Returns the result."""
    dev = {k: _utf8(v) for k, v in cols.items()}
    entries = list(numeric) + [("STRING_AGG",) + dev[c] + (sep,) for c, sep in aggs]
    out = eng.merge_agg(_side(chrom, start, end), n_chrom, distance, entries, preds=preds)
    ref = S.merge_string_agg(np.asarray(chrom).tolist(), np.asarray(start).tolist(), np.asarray(end).tolist(), distance,
                             cols, aggs, holds)
    assert len(out) == 4 + len(entries)
    assert [t.cpu().tolist() for t in out[:4]] == [[row[k] for row in ref] for k in range(4)]
    for j in range(len(aggs)):
        got = _decode(*out[4 + len(numeric) + j])
        assert got == [row[4 + j] for row in ref], (aggs[j], [g for g, (a, b) in enumerate(zip(got, (row[4 + j] for row in ref))) if a != b][:5])
    return out


def _random_table(r, n, n_part=5):
    chrom = r.integers(0, n_part, n)
    start = r.integers(0, max(20 * n // n_part, 50), n)
    return chrom, start, start + r.integers(1, 60, n)


def _built_regions(r, lengths, shuffle=True):
    """One partition whose merged regions have exactly ``lengths`` rows (regions lie 6000 apart, every interval of a
    region overlaps the others).  Returns chrom, start, end, the region and the rank inside it (by start) per row."""
    start = np.concatenate([6000 * j + np.arange(L) for j, L in enumerate(lengths)])
    end = np.concatenate([np.full(L, 6000 * j + 5500) for j, L in enumerate(lengths)])
    region = np.concatenate([np.full(L, j) for j, L in enumerate(lengths)])
    rank = np.concatenate([np.arange(L) for L in lengths])
    order = r.permutation(len(start)) if shuffle else np.arange(len(start))
    return np.zeros(len(start), np.int64), start[order], end[order], region[order], rank[order]


# ------------------------------------------------------------------------------------------ HipEngine.merge_agg
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1000, 5000])
def test_random_tables(eng, n):
    r = np.random.default_rng(200 + n)
    chrom, start, end = _random_table(r, n)
    cols = {"name": _values(r, n, lengths=LENGTHS if n <= 1000 else LENGTHS[:-3])}
    run_and_check(eng, chrom, start, end, 5, 0, cols, [("name", b",")])
    run_and_check(eng, chrom, start, end, 5, 30, cols, [("name", b"; ")])          # distance > 0


@pytest.mark.parametrize("lengths", [
    [63], [64], [65], [NT - 1], [NT], [NT + 1], [SCAN - 1], [SCAN], [SCAN + 1],          # one region = all n rows
    [3, 64, 5], [3, 65, 5], [1, NT, 2], [7, NT + 1, 1], [NT - 1, 1, NT, 1, NT + 1],
    [63, 1, 64, 1, 65, 127, 129],                                                      # regions start / end on wave edges
    [5, SCAN - 5, 9], [5, SCAN - 6, 9], [5, SCAN - 4, 9], [SCAN, SCAN, 1], [SCAN - 1, 2, SCAN - 1],
], ids=lambda v: "-".join(map(str, v)))
def test_region_length_edges(eng, lengths):
    r = np.random.default_rng(21)
    chrom, start, end, _region, _rank = _built_regions(r, lengths)
    out = run_and_check(eng, chrom, start, end, 1, 0, {"name": _values(r, len(start), nulls=0.2)}, [("name", b"+")])
    assert out[3].cpu().tolist() == lengths


@pytest.mark.parametrize("sep", SEPARATORS, ids=lambda s: f"sep{len(s)}")
def test_every_value_length_with_every_separator(eng, sep):
    r = np.random.default_rng(22)
    n = 30 * len(LENGTHS)
    chrom, start, end = _random_table(r, n, 3)
    names = [_word(r, LENGTHS[i % len(LENGTHS)], i) for i in range(n)]
    for i in r.choice(n, n // 10, replace=False):
        names[i] = None
    run_and_check(eng, chrom, start, end, 3, 15, {"name": names}, [("name", sep)])


@pytest.mark.parametrize("sep", [b"", b"/"], ids=["nosep", "sep"])
def test_null_placement_inside_a_region(eng, sep):
    r = np.random.default_rng(23)
    lengths = [5, 70, 1, 300, 2, 66, 4, 130]
    chrom, start, end, region, rank = _built_regions(r, lengths)
    names = [_word(r, 6, i) for i in range(len(start))]

    def null(rows):
        for i in np.nonzero(rows)[0]:
            names[i] = None

    null((region == 0) & (rank == 0))                   # NULL first
    null((region == 1) & (rank == lengths[1] - 1))      # NULL last
    null((region == 2))                                 # a one-row region that is NULL
    null((region == 3) & (rank != 150))                 # exactly one non-NULL, in the middle of 300
    null((region == 4))                                 # all NULL
    null((region == 5) & (rank < 65))                   # exactly one non-NULL, last, past a wave
    null((region == 6) & (rank > 0))                    # exactly one non-NULL, first
    null((region == 7) & (rank % 2 == 0))               # every other one
    out = run_and_check(eng, chrom, start, end, 1, 0, {"name": names}, [("name", sep)])
    assert out[4][2].cpu().tolist() == [True, True, False, True, False, True, True, True]


@pytest.mark.parametrize("sep", [b"", b"-"], ids=["nosep", "sep"])
def test_empty_strings_are_values_and_nulls_are_not(eng, sep):
    r = np.random.default_rng(24)
    chrom, start, end, region, _rank = _built_regions(r, [4, 90, 3, 3, 260])
    names = []
    for g in region:
        names.append({0: b"", 1: r.choice([b"", None]), 2: None, 3: r.choice([b"", b"x", None])}.get(int(g), r.choice([b"", b"ab", None])))
    names = [None if v is None else bytes(v) for v in names]
    out = _decode(*run_and_check(eng, chrom, start, end, 1, 0, {"name": names}, [("name", sep)])[4])
    assert out[0] == sep * 3 and out[2] is None          # only empty strings: a run of separators, and valid


def test_equal_starts_keep_the_row_order(eng):
    r = np.random.default_rng(25)
    n = 3000
    chrom = r.integers(0, 2, n)
    start = r.integers(0, 40, n)                         # ~37 rows per (chrom, start)
    end = start + r.integers(1, 5, n)
    names = [b"r%d" % i for i in range(n)]
    out = _decode(*run_and_check(eng, chrom, start, end, 2, 0, {"name": names}, [("name", b",")])[4])
    ids = [int(t[1:]) for t in out[0].split(b",")]
    assert any(a > b for a, b in zip(ids, ids[1:])) and len(ids) > 1000          # not simply ascending row ids


@pytest.mark.parametrize("form, env, local", [
    ("four_pass", {"GIQL_HIP_LOCAL_MIN_ROWS": "1", "GIQL_HIP_NO_LOCAL_SORT": "1"}, False),
    ("local16", {"GIQL_HIP_LOCAL_MIN_ROWS": "1"}, True),
    ("local13", {"GIQL_HIP_LOCAL_MIN_ROWS": "1", "GIQL_HIP_LOCAL_BITS": "13"}, True),
])
def test_every_sort_form_keeps_start_then_row_order(form, env, local):
    """The merge's sort by start in its two forms -- four global passes, or global passes over the key's high bits and
    one LDS bucket stage -- with equal starts in every bucket.  The second call speculates on the first one's span."""
    e = _engine(env)
    try:
        r = np.random.default_rng(26)
        n = 3000
        chrom, start = np.zeros(n, np.int64), r.integers(0, 60, n) * 1000
        end = start + r.integers(1, 900, n)
        names = [b"r%d" % i for i in range(n)]
        for _call in range(2):
            run_and_check(e, chrom, start, end, 1, 0, {"name": names}, [("name", b",")])
        e.merge(_side(chrom, start, end), 1, 0)
        print(f"\n[{form}] sort_local={e.stats()['sort_local']} bucket_bits={e.stats()['bucket_bits']}")
        assert e.stats()["sort_local"] == local
    finally:
        e.close()


def test_predicate_regions(eng):
    r = np.random.default_rng(27)
    n = 2000
    start = np.sort(r.choice(60_000, n, replace=False))
    end = start + r.integers(20, 400, n)
    end[0] = 70_000                                      # every region ends under a longer shadow
    depth = np.repeat(r.permutation(n // 150 + 1), 150)[:n].astype(np.int64)
    order = r.permutation(n)
    start, end, depth = start[order], end[order], depth[order]
    d = _dev(depth)
    out = run_and_check(eng, np.zeros(n, np.int64), start, end, 1, 0, {"name": _values(r, n)}, [("name", b",")],
                        preds=[(("a", d), "=", ("b", d))], holds=lambda i, j: depth[i] == depth[j])
    assert int(out[0].numel()) >= n // 150 and int(out[3].max()) >= 150


def test_a_genome_wider_than_the_32_bit_axis(eng):
    from giql_amd import _lib

    r = np.random.default_rng(28)
    n = 700
    chrom = r.integers(0, 2, n)
    start = np.where(r.random(n) < 0.5, r.integers(0, 40_000, n), 2_147_000_000 + r.integers(0, 40_000, n))
    end = start + r.integers(1, 600, n)
    chrom[:4] = [0, 0, 1, 1]                             # each chromosome spans [0, 2^31 - 1] exactly: 2^32 in all
    start[:4], end[:4] = [0, 2**31 - 101] * 2, [100, 2**31 - 1] * 2
    names = _values(r, n, lengths=LENGTHS[:12])
    off, data, valid = _utf8(names)
    with pytest.raises(_lib.GiqlHipError) as exc:
        eng._merge_agg_once(_side(chrom, start, end), 2, 0, [("STRING_AGG", off, data, valid, b",")])
    assert exc.value.code == _lib.GIQL_ERR_SPAN
    score = _dev(r.integers(-50, 50, n))
    out = run_and_check(eng, chrom, start, end, 2, 0, {"name": names}, [("name", b","), ("name", b"")],
                        numeric=[("SUM", score, None)])
    plain = eng.merge_agg(_side(chrom, start, end), 2, 0, [("SUM", score, None)])
    assert torch.equal(out[4][0], plain[4][0]) and torch.equal(out[4][1], plain[4][1])


def test_two_columns_and_one_column_twice_beside_sum_and_count(eng):
    r = np.random.default_rng(29)
    n = 3000
    chrom, start, end = _random_table(r, n)
    cols = {"a": _values(r, n, lengths=LENGTHS[:14]), "b": _values(r, n, nulls=0.6)}
    score, ok = _dev(r.normal(0, 100, n)), _dev((r.random(n) > 0.3).astype(np.uint8))
    weight = _dev(r.integers(-9, 9, n).astype(np.int32))
    numeric = [("SUM", score, ok), ("COUNT", weight, None), ("AVG", score, ok)]
    out = run_and_check(eng, chrom, start, end, 5, 10, cols, [("a", b","), ("b", b" | "), ("a", b""), ("b", "→".encode())],
                        numeric=numeric)
    plain = eng.merge_agg(_side(chrom, start, end), 5, 10, numeric)
    for j in range(3):
        assert torch.equal(out[4 + j][1], plain[4 + j][1])
        assert torch.equal(out[4 + j][0].view(torch.int64), plain[4 + j][0].view(torch.int64))      # the same bits


def test_the_caps_and_the_entry_checks(eng):
    r = np.random.default_rng(30)
    n = 100
    chrom, start, end = _random_table(r, n)
    side = _side(chrom, start, end)
    off, data, valid = _utf8(_values(r, n))
    s = ("STRING_AGG", off, data, valid, ",")
    v = _dev(r.normal(size=n))
    assert len(eng.merge_agg(side, 5, 0, [s] * 4 + [("SUM", v, None)] * 4)) == 12
    for bad in ([s] * 5, [s] + [("SUM", v, None)] * 8):
        with pytest.raises(ValueError, match="at most 8 aggregates, 4 of them STRING_AGG"):
            eng.merge_agg(side, 5, 0, bad)
    with pytest.raises(ValueError, match="separator of 256 bytes"):
        eng.merge_agg(side, 5, 0, [("STRING_AGG", off, data, valid, "x" * 256)])
    with pytest.raises(ValueError, match="one entry per row plus one"):
        eng.merge_agg(side, 5, 0, [("STRING_AGG", off[:-1].contiguous(), data, valid, ",")])
    with pytest.raises(ValueError, match="STRING_AGG entry is"):
        eng.merge_agg(side, 5, 0, [("STRING_AGG", off, data, valid)])


def test_an_empty_table(eng):
    z = np.zeros(0, np.int32)
    off, data, valid = _utf8([])
    out = eng.merge_agg(_side(z, z, z), 1, 0, [("STRING_AGG", off, data, valid, ","), ("COUNT", _dev(z), None)])
    assert [int(t.numel()) for t in out[:4]] == [0] * 4
    assert out[4][0].cpu().tolist() == [0] and int(out[4][1].numel()) == 0 and int(out[4][2].numel()) == 0
    assert int(out[5][0].numel()) == 0


def test_the_same_call_twice_returns_the_same_bytes(eng):
    r = np.random.default_rng(31)
    chrom, start, end = _random_table(r, 5000)
    start = start // 8 * 8                               # plenty of equal starts
    side = _side(chrom, start, start + 20)
    off, data, valid = _utf8(_values(r, 5000, lengths=LENGTHS[:15]))
    first = eng.merge_agg(side, 5, 40, [("STRING_AGG", off, data, valid, ", ")])[4]
    again = eng.merge_agg(side, 5, 40, [("STRING_AGG", off, data, valid, ", ")])[4]
    assert all(torch.equal(a, b) for a, b in zip(first, again))


# ---------------------------------------------------------------------------------------------- execute()
def _golden_table(pa):
    rows = GOLDEN["rows"]
    types = [pa.string(), pa.int32(), pa.int32(), pa.string(), pa.string()]
    return pa.table({c: pa.array([r[k] for r in rows], type=t) for k, (c, t) in enumerate(zip(GOLDEN["columns"], types))})


def _tokens(s, sep):
    return None if s is None else sorted(collections.Counter(s.split(sep)).items())


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=lambda c: c["name"])
def test_execute_returns_the_sqlite_minted_rows(eng, case):
    pa = pytest.importorskip("pyarrow")
    from giql_amd.execute import execute

    sep, rows = GOLDEN["separator"], GOLDEN["rows"]
    args = "interval" + (f", {case['distance']}" if case["distance"] else "") + (", stranded := true" if case["stranded"] else "")
    keys = ["chrom"] + (["strand"] if case["stranded"] else []) + ["start", "end"]
    k = len(keys)
    out = execute(f"SELECT MERGE({args}), COUNT(*) AS n, STRING_AGG(name, '{sep}') AS names FROM features",
                  {"features": _golden_table(pa)}, eng, giql_tables=["features"], string_aggregates=True)
    assert out.column_names == keys + ["n", "names"] and out.schema.field("names").type == pa.string()
    got = [list(row) for row in zip(*(out.column(c).to_pylist() for c in out.column_names))]
    assert [(x[0], x[k - 2]) for x in got] == sorted((x[0], x[k - 2]) for x in got)       # ORDER BY chrom, start
    by_key = lambda x: (x[0], x[k - 2], x[1])
    # sqlite's rows, as token multisets
    want = [row[:k + 1] + [_tokens(row[k + 2], sep)] for row in case["merged"]]
    assert sorted((x[:k + 1] + [_tokens(x[k + 1], sep)] for x in got), key=by_key) == sorted(want, key=by_key)
    # the restatement's, exactly
    part = [(r[0], r[3]) if case["stranded"] else (r[0],) for r in rows]
    ref = S.merge_string_agg(part, [r[1] for r in rows], [r[2] for r in rows], case["distance"],
                             {"name": [r[4] for r in rows]}, [("name", sep)])
    assert sorted(got, key=by_key) == sorted(([*x[0], *x[1:]] for x in ref), key=by_key)


def test_execute_the_documented_recipe(eng):
    pa = pytest.importorskip("pyarrow")
    from giql_amd.execute import execute

    recipe = """SELECT
       MERGE(interval),
       STRING_AGG(name, ',') AS merged_features
   FROM features"""
    rows = GOLDEN["rows"]
    tbl = _golden_table(pa)
    out = execute(recipe, {"features": tbl}, eng, giql_tables=["features"], string_aggregates=True)
    ref = S.merge_string_agg([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], 0,
                             {"name": [r[4] for r in rows]}, [("name", ",")])
    assert out.column_names == ["chrom", "start", "end", "merged_features"]
    assert [list(x) for x in zip(*(out.column(c).to_pylist() for c in out.column_names))] == [x[:3] + x[4:] for x in ref]
    assert out.column("merged_features").null_count > 0
    # without the keyword the query string declines; a plan string made with it runs as it is
    from giql_amd.transpile import HipDeclined, transpile
    with pytest.raises(HipDeclined):
        execute(recipe, {"features": tbl}, eng, giql_tables=["features"])
    with pytest.raises(HipDeclined, match="STRING_AGG beside MERGE"):
        execute(recipe, {"features": tbl}, eng, giql_tables=["features"], merge_aggregates=True)
    text = transpile(recipe, ["features"], dialect="hip", string_aggregates=True)
    assert execute(text, {"features": tbl}, eng).equals(out)
    with pytest.raises(ValueError, match="return_indices"):
        execute(recipe, {"features": tbl}, eng, giql_tables=["features"], string_aggregates=True, return_indices=True)
    with pytest.raises(ValueError, match="column 'start' has type int32"):
        execute("SELECT MERGE(interval), STRING_AGG(start, ',') AS s FROM features", {"features": tbl}, eng,
                giql_tables=["features"], string_aggregates=True)


def _arrow_case(pa, r, n, n_part=3):
    chrom, start, end = _random_table(r, n, n_part)
    names = [None if v is None else v.decode() for v in _values(r, n, lengths=LENGTHS[:13])]
    tbl = pa.table({"chrom": pa.array([f"chr{c + 1}" for c in chrom]), "start": pa.array(start, pa.int32()),
                    "end": pa.array(end, pa.int32()), "name": pa.array(names, pa.string())})
    return tbl, [f"chr{c + 1}" for c in chrom], start, end, names


def _rows(out):
    return [list(x) for x in zip(*(out.column(c).to_pylist() for c in out.column_names))]


def test_execute_behind_a_where_and_mixed_with_numeric_aggregates(eng):
    pa = pytest.importorskip("pyarrow")
    from giql_amd.execute import execute

    r = np.random.default_rng(32)
    n = 3000
    tbl, chrom, start, end, names = _arrow_case(pa, r, n)
    depth = r.integers(0, 4, n)
    score = r.integers(-100, 100, n)
    tbl = tbl.append_column("depth", pa.array(depth)).append_column("score", pa.array(score))
    out = execute("SELECT MERGE(interval, 10), SUM(score) AS total, STRING_AGG(name, '; ') AS names, COUNT(*) AS n, "
                  "STRING_AGG(name, '') AS glued FROM t WHERE depth < 2", {"t": tbl}, eng, giql_tables=["t"],
                  merge_aggregates=True, string_aggregates=True)
    keep = np.nonzero(depth < 2)[0]
    assert 0 < len(keep) < n
    kept = {"name": [names[i] for i in keep]}
    ref = S.merge_string_agg([chrom[i] for i in keep], start[keep].tolist(), end[keep].tolist(), 10, kept,
                             [("name", "; "), ("name", "")])
    sums = R.merge_agg([chrom[i] for i in keep], start[keep].tolist(), end[keep].tolist(), 10,
                       {"score": [int(score[i]) for i in keep]}, [("SUM", "score")])
    assert out.column_names == ["chrom", "start", "end", "total", "names", "n", "glued"]
    assert _rows(out) == [[x[0], x[1], x[2], s[4], x[4], x[3], x[5]] for x, s in zip(ref, sums)]


def test_execute_sliced_large_and_dictionary_columns(eng):
    pa = pytest.importorskip("pyarrow")
    from giql_amd.execute import execute

    r = np.random.default_rng(33)
    n = 1200
    tbl, chrom, start, end, names = _arrow_case(pa, r, n + 57)
    sliced = tbl.slice(57)                               # non-zero array offset, offsets[0] != 0
    assert sliced.column("name").chunk(0).offset == 57
    ref = S.merge_string_agg(chrom[57:], start[57:].tolist(), end[57:].tolist(), 0, {"name": names[57:]}, [("name", "|")])
    query = "SELECT MERGE(interval), STRING_AGG(name, '|') AS names FROM t"
    want = [x[:3] + x[4:] for x in ref]
    assert _rows(execute(query, {"t": sliced}, eng, giql_tables=["t"], string_aggregates=True)) == want
    for other_name in (sliced.column("name").cast(pa.large_string()), sliced.column("name").dictionary_encode()):
        other = sliced.set_column(sliced.column_names.index("name"), "name", other_name)
        assert other.schema.field("name").type != pa.string()
        out = execute(query, {"t": other}, eng, giql_tables=["t"], string_aggregates=True)
        assert out.schema.field("names").type == pa.string() and _rows(out) == want
    chunked = pa.concat_tables([sliced.slice(0, 500), sliced.slice(500)])
    assert chunked.column("name").num_chunks == 2
    assert _rows(execute(query, {"t": chunked}, eng, giql_tables=["t"], string_aggregates=True)) == want


def test_execute_stranded_keeps_the_final_order(eng):
    pa = pytest.importorskip("pyarrow")
    from giql_amd.execute import execute

    r = np.random.default_rng(34)
    n = 1500
    tbl, chrom, start, end, names = _arrow_case(pa, r, n)
    strand = r.choice(["+", "-"], n).tolist()
    tbl = tbl.append_column("strand", pa.array(strand))
    out = execute("SELECT MERGE(interval, stranded := true), STRING_AGG(name, ',') AS names FROM t", {"t": tbl}, eng,
                  giql_tables=["t"], string_aggregates=True)
    ref = S.merge_string_agg(list(zip(chrom, strand)), start.tolist(), end.tolist(), 0, {"name": names}, [("name", ",")])
    got = _rows(out)
    assert out.column_names == ["chrom", "strand", "start", "end", "names"]
    assert [(x[0], x[2]) for x in got] == sorted((x[0], x[2]) for x in got)
    key = lambda x: (x[0], x[2], x[1])
    assert sorted(got, key=key) == sorted(([*x[0], x[1], x[2], x[4]] for x in ref), key=key)


def test_execute_a_genome_wider_than_the_32_bit_axis(eng):
    pa = pytest.importorskip("pyarrow")
    from giql_amd.execute import execute

    r = np.random.default_rng(35)
    n = 600
    chrom = [f"chr{c}" for c in r.integers(0, 2, n)]
    start = np.where(r.random(n) < 0.5, r.integers(0, 40_000, n), 2_147_000_000 + r.integers(0, 40_000, n))
    end = start + r.integers(1, 600, n)
    chrom[:4] = ["chr0", "chr0", "chr1", "chr1"]
    start[:4], end[:4] = [0, 2**31 - 101] * 2, [100, 2**31 - 1] * 2
    names = [None if v is None else v.decode() for v in _values(r, n)]
    tbl = pa.table({"chrom": pa.array(chrom), "start": pa.array(start, pa.int32()), "end": pa.array(end, pa.int32()),
                    "name": pa.array(names, pa.string())})
    out = execute("SELECT MERGE(interval), STRING_AGG(name, ',') AS names FROM t", {"t": tbl}, eng, giql_tables=["t"],
                  string_aggregates=True)
    ref = S.merge_string_agg(chrom, start.tolist(), end.tolist(), 0, {"name": names}, [("name", ",")])
    assert _rows(out) == [x[:3] + x[4:] for x in ref]


# ---------------------------------------------------------------------------------------------- the C ABI
def _guarded(n_bytes):
    """``n_bytes`` of device memory followed by a 64-byte tail, all 0xAA."""
    return torch.full((n_bytes + 64,), AA, dtype=torch.uint8, device="cuda:0")


def _tail_intact(t, n_bytes):
    return bool((t[n_bytes:] == AA).all())


class RawCall:
    """One ``giql_hip_merge_str_dev`` through ctypes over ``cols = [(offsets, valid | None, sep_len)]``, every output of
    the string aggregates exactly as large as the header says plus a guarded tail."""

    def __init__(self, eng, side, n_chrom, distance, cols, capacity):
        from giql_amd import _lib

        n = side.n
        self.n, self.cap, self.side = n, capacity, side
        self.fixed = [torch.zeros(max(capacity, 1), dtype=torch.int32, device="cuda:0") for _ in range(3)]
        self.count = torch.zeros(max(capacity, 1), dtype=torch.int64, device="cuda:0")
        self.order = _guarded(4 * n)
        self.bufs = [(_guarded(4 * (capacity + 1)), _guarded(8 * capacity), _guarded(4 * n)) for _ in cols]
        self.strs = (_lib.CStrAgg * max(len(cols), 1))()
        for j, (off, valid, sep_len) in enumerate(cols):
            o, nn, dst = self.bufs[j]
            self.strs[j] = _lib.CStrAgg(off.data_ptr(), None if valid is None else valid.data_ptr(), sep_len,
                                        o.data_ptr(), nn.data_ptr(), dst.data_ptr(), -7)
        self.m = ctypes.c_int64(-1)
        self.rc = eng._L.giql_hip_merge_str_dev(
            eng._h, side.c_struct(), n_chrom, distance, None, 0, None, 0, self.strs, len(cols), self.fixed[0].data_ptr(),
            self.fixed[1].data_ptr(), self.fixed[2].data_ptr(), self.count.data_ptr(), self.order.data_ptr(), capacity,
            ctypes.byref(self.m), eng._stream())
        self.error = eng._L.giql_hip_last_error()

    def tails_intact(self):
        return _tail_intact(self.order, 4 * self.n) and all(
            _tail_intact(o, 4 * (self.cap + 1)) and _tail_intact(nn, 8 * self.cap) and _tail_intact(dst, 4 * self.n)
            for o, nn, dst in self.bufs)

    def fill(self, eng, j, off, data, sep, order=None, n_rows=None):
        """(return code, guarded output) of ``giql_hip_concat_utf8_fill_dev`` for aggregate ``j``."""
        out = _guarded(max(int(self.strs[j].n_bytes), 0))
        rc = eng._L.giql_hip_concat_utf8_fill_dev(
            eng._h, off.data_ptr(), data.data_ptr(), self.n if n_rows is None else n_rows,
            (self.order if order is None else order).data_ptr(), self.bufs[j][2].data_ptr(), self.n, sep, len(sep),
            out.data_ptr(), eng._stream())
        return rc, out


def test_the_outputs_stay_inside_their_buffers(eng):
    r = np.random.default_rng(36)
    n = 2500
    chrom, start, end = _random_table(r, n)
    names = _values(r, n, lengths=LENGTHS)
    seps = [b",", b"0123456789abcdefg"]
    ref = S.merge_string_agg(chrom.tolist(), start.tolist(), end.tolist(), 0, {"name": names}, [("name", s) for s in seps])
    m = len(ref)
    off, data, valid = _utf8(names)
    call = RawCall(eng, _side(chrom, start, end), 5, 0, [(off, valid, len(s)) for s in seps], m)
    assert call.rc == 0, call.error
    assert int(call.m.value) == m and call.tails_intact()
    order = call.order[:4 * n].view(torch.int32).cpu().numpy()
    assert sorted(order.tolist()) == list(range(n))
    # region r owns out_count[r] consecutive entries of the order, in (start, row) order
    first = np.concatenate([[0], np.cumsum(call.count[:m].cpu().numpy())])
    regions = R.regions(chrom.tolist(), start.tolist(), end.tolist(), 0)
    assert [order[first[g]:first[g + 1]].tolist() for g in range(m)] == [S.members_in_order(mem, start) for _p, mem in regions]
    for j, sep in enumerate(seps):
        o, nn, dst = call.bufs[j]
        offsets = o[:4 * (m + 1)].view(torch.int32)
        assert int(call.strs[j].n_bytes) == int(offsets[-1]) == sum(len(x[4 + j] or b"") for x in ref)
        assert nn[:8 * m].view(torch.int64).cpu().tolist() == [sum(names[i] is not None for i in mem) for _p, mem in regions]
        words = dst[:4 * n].view(torch.int32).cpu().numpy().view(np.uint32)
        assert [(w == 0xFFFFFFFF) for w in words] == [names[i] is None for i in order]
        rc, out = call.fill(eng, j, off, data, sep)
        assert rc == 0 and _tail_intact(out, int(call.strs[j].n_bytes))
        got = _decode(offsets, out[:int(call.strs[j].n_bytes)], nn[:8 * m].view(torch.int64) > 0)
        assert got == [x[4 + j] for x in ref]
    assert call.tails_intact()


def test_argument_errors_name_the_aggregate_and_launch_nothing():
    from giql_amd import _lib

    e = _engine()
    try:
        r = np.random.default_rng(37)
        n = 64
        chrom, start, end = _random_table(r, n)
        side = _side(chrom, start, end)
        off, data, valid = _utf8(_values(r, n))
        good = (off, valid, 1)
        for cols, k_strs, message in (([good] * 0, 0, b"0 string aggregates"), ([good] * 4, 5, b"5 string aggregates"),
                                      ([good, (off, valid, 256)], 2, b"string aggregate 1: separator of 256 bytes"),
                                      ([good, good, (off, valid, -1)], 3, b"string aggregate 2: separator of -1 bytes")):
            strs = (_lib.CStrAgg * 5)()
            for j, (o, v, sl) in enumerate(cols):
                strs[j] = _lib.CStrAgg(o.data_ptr(), None, sl, o.data_ptr(), o.data_ptr(), o.data_ptr(), 0)
            m = ctypes.c_int64(-1)
            rc = e._L.giql_hip_merge_str_dev(e._h, side.c_struct(), 5, 0, None, 0, None, 0, strs, k_strs, off.data_ptr(),
                                             off.data_ptr(), off.data_ptr(), None, off.data_ptr(), n, ctypes.byref(m), None)
            assert rc == _lib.GIQL_ERR_INVALID and message in e._L.giql_hip_last_error(), e._L.giql_hip_last_error()
        scratch = torch.zeros(8 * (n + 1), dtype=torch.uint8, device="cuda:0")
        for field in ("offsets", "out_offsets", "out_nn", "row_dst"):
            strs = (_lib.CStrAgg * 2)()
            for j in range(2):
                strs[j] = _lib.CStrAgg(off.data_ptr(), None, 1, scratch.data_ptr(), scratch.data_ptr(), scratch.data_ptr(), 0)
            setattr(strs[1], field, None)
            m = ctypes.c_int64(-1)
            rc = e._L.giql_hip_merge_str_dev(e._h, side.c_struct(), 5, 0, None, 0, None, 0, strs, 2, off.data_ptr(),
                                             off.data_ptr(), off.data_ptr(), None, scratch.data_ptr(), n, ctypes.byref(m), None)
            assert rc == _lib.GIQL_ERR_INVALID and b"string aggregate 1:" in e._L.giql_hip_last_error(), field
        rc = e._L.giql_hip_merge_str_dev(e._h, side.c_struct(), 5, 0, None, 0, None, 0, strs, 1, off.data_ptr(),
                                         off.data_ptr(), off.data_ptr(), None, None, n, ctypes.byref(m), None)
        assert rc == _lib.GIQL_ERR_INVALID and b"out_order is NULL" in e._L.giql_hip_last_error()
        rc = e._L.giql_hip_merge_str_dev(e._h, side.c_struct(), 5, 0, None, 0, None, 9, strs, 1, off.data_ptr(),
                                         off.data_ptr(), off.data_ptr(), None, scratch.data_ptr(), n, ctypes.byref(m), None)
        assert rc == _lib.GIQL_ERR_INVALID and b"9 aggregates" in e._L.giql_hip_last_error()
        for sep_len, sep in ((256, b"x" * 256), (-1, b""), (3, None)):
            rc = e._L.giql_hip_concat_utf8_fill_dev(e._h, off.data_ptr(), data.data_ptr(), n, off.data_ptr(), off.data_ptr(),
                                                    n, sep, sep_len, scratch.data_ptr(), None)
            assert rc == _lib.GIQL_ERR_INVALID and b"separator" in e._L.giql_hip_last_error()
        assert sum(e.stats()["phase_launches"].values()) == 0          # nothing was launched by any of them
    finally:
        e.close()


def test_capacity_names_the_aggregate_whose_output_passes_int32(eng):
    """Three rows of one region whose offsets claim 2^31 - 1 bytes in all: the plan reads offsets only, no byte moves.
    With no separator the output fits exactly; with one it is two bytes over (a region past the limit counts as 2^31
    bytes: the size in the message is a lower bound)."""
    from giql_amd import _lib

    z = np.zeros(3, np.int64)
    side = _side(z, [10, 11, 12], [50, 50, 50])
    off = _dev(np.array([0, 2**30, 2**31 - 2, 2**31 - 1], np.int32))
    call = RawCall(eng, side, 1, 0, [(off, None, 0), (off, None, 1), (off, None, 0)], 3)
    assert call.rc == _lib.GIQL_ERR_CAPACITY and b"string aggregate 1: output of 2147483648 bytes or more" in call.error
    assert [int(s.n_bytes) for s in call.strs] == [2**31 - 1, -1, 2**31 - 1] and int(call.m.value) == 1
    assert call.tails_intact()


def test_a_decreasing_offset_pair_and_an_order_past_the_column_are_refused(eng):
    from giql_amd import _lib

    r = np.random.default_rng(38)
    n = 300
    chrom, start, end = _random_table(r, n)
    names = _values(r, n, nulls=0.0)
    off, data, _valid = _utf8(names)
    side = _side(chrom, start, end)
    m = len(R.regions(chrom.tolist(), start.tolist(), end.tolist(), 0))
    bad = off.clone()
    bad[200] = int(off[199]) - 1 if int(off[199]) > 0 else -1          # row 199 ends before it begins
    call = RawCall(eng, side, 5, 0, [(off, None, 1), (bad, None, 1)], m)
    assert call.rc == _lib.GIQL_ERR_INVALID and b"string aggregate 1: an offset pair" in call.error
    assert call.tails_intact()
    good = RawCall(eng, side, 5, 0, [(off, None, 1)], m)
    assert good.rc == 0
    order = good.order[:4 * n].view(torch.int32).clone()
    order[17] = n                                                      # one past the column
    rc, out = good.fill(eng, 0, off, data, b",", order=order)
    assert rc == _lib.GIQL_ERR_INVALID and b"concat_utf8_fill" in eng._L.giql_hip_last_error()
    assert _tail_intact(out, int(good.strs[0].n_bytes))
    rc, out = good.fill(eng, 0, off, data, b",")
    assert rc == 0


# ------------------------------------------------------------------ the plan-lifetime cells of the two entry points
KINDS = ("INNER", "WINDOW", "DISJOIN", "CONTAINS")


class Plans:
    def __init__(self, eng):
        r = np.random.default_rng(39)
        self.eng, self.L, self.h = eng, eng._L, eng._h
        self.a = _side(*self._table(r, 300))
        self.b = _side(*self._table(r, 200))

    @staticmethod
    def _table(r, n):
        chrom = r.integers(0, 3, n)
        start = r.integers(0, 3000, n)
        return chrom, start, start + r.integers(1, 80, n)

    def plan(self, kind):
        n = ctypes.c_int64(-1)
        x, y, st = self.a.c_struct(), self.b.c_struct(), self.eng._stream()
        if kind == "INNER":
            rc = self.L.giql_hip_inner_plan_dev(self.h, x, y, 3, st, ctypes.byref(n))
        elif kind == "WINDOW":
            rc = self.L.giql_hip_window_plan_dev(self.h, x, y, 3, 50, st, ctypes.byref(n))
        elif kind == "DISJOIN":
            rc = self.L.giql_hip_disjoin_plan_dev(self.h, x, y, 3, ctypes.byref(n), st)
        else:
            rc = self.L.giql_hip_contain_plan_dev(self.h, x, y, 3, st, ctypes.byref(n))
        assert rc == 0 and n.value > 0, (kind, rc, n.value)
        return int(n.value)

    def fill(self, kind, cap):
        outs = [torch.full((cap + 8,), -7, dtype=torch.int32, device="cuda:0") for _ in range(3 if kind == "DISJOIN" else 2)]
        p, st = [o.data_ptr() for o in outs], self.eng._stream()
        if kind in ("INNER", "WINDOW"):
            rc = self.L.giql_hip_inner_fill_dev(self.h, p[0], p[1], cap, st)
        elif kind == "DISJOIN":
            rc = self.L.giql_hip_disjoin_fill_dev(self.h, p[0], p[1], p[2], cap, st)
        else:
            rc = self.L.giql_hip_contain_fill_dev(self.h, p[0], p[1], cap, st)
        return rc, outs


@pytest.mark.parametrize("n_rows", [64, 0], ids=["rows", "no_rows"])
@pytest.mark.parametrize("kind", KINDS)
def test_merge_str_drops_a_plan_the_context_keeps(eng, kind, n_rows):
    """``giql_hip_merge_str_dev`` begins a call: whatever plan the context keeps is dropped -- its fill answers
    GIQL_ERR_STATE and writes nothing -- also when the table is empty."""
    from giql_amd import _lib

    plans = Plans(eng)
    cap = plans.plan(kind)
    rc, outs = plans.fill(kind, cap)
    assert rc == 0 and int((outs[0] != -7).sum()) == cap
    r = np.random.default_rng(40)
    chrom, start, end = _random_table(r, n_rows)
    off, _data, valid = _utf8(_values(r, n_rows))
    call = RawCall(eng, _side(chrom, start, end), 5, 0, [(off, valid, 1)], n_rows)
    assert call.rc == 0 and (n_rows or (int(call.m.value) == 0 and int(call.strs[0].n_bytes) == 0))
    rc, outs = plans.fill(kind, cap)
    assert rc == _lib.GIQL_ERR_STATE and all(bool((o == -7).all()) for o in outs)


@pytest.mark.parametrize("kind", KINDS)
def test_the_fill_keeps_a_join_plan_and_drops_a_contains_plan(eng, kind):
    """``giql_hip_concat_utf8_fill_dev`` uses no workspace: an INNER, WINDOW or DISJOIN plan survives it (their fill
    still succeeds); a CONTAINS plan goes, as with ``giql_hip_take_utf8_fill_dev``."""
    from giql_amd import _lib

    r = np.random.default_rng(41)
    chrom, start, end = _random_table(r, 500)
    off, data, valid = _utf8(_values(r, 500))
    call = RawCall(eng, _side(chrom, start, end), 5, 0, [(off, valid, 2)], 500)
    assert call.rc == 0
    plans = Plans(eng)
    cap = plans.plan(kind)
    rc, out = call.fill(eng, 0, off, data, b"::")
    assert rc == 0 and _tail_intact(out, int(call.strs[0].n_bytes))
    rc, outs = plans.fill(kind, cap)
    if kind == "CONTAINS":
        assert rc == _lib.GIQL_ERR_STATE and all(bool((o == -7).all()) for o in outs)
    else:
        assert rc == 0 and int((outs[0] != -7).sum()) == cap
