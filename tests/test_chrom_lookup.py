"""The chrom lookup of the indexed ``execute()`` path (``execute._chrom_lookup``) matches two columns the way the
ordinary join's ``encode_chroms`` does -- no GPU needed.  The GPU-side parity of the three paths (pinned with an
index, pinned, unpinned) is ``tests/test_index_gpu.py::test_indexed_execute_matches_the_ordinary_join_for_every_chrom_kind``."""

import numpy as np
import pytest

from giql_amd.execute import _chrom_lookup, _chrom_values, encode_chroms


def _lookup_like_encode_chroms(index_col, query_col):
    """What the ordinary join makes of the same two columns: for every query row, the index row position of its
    chromosome in the index's own dictionary (or len(dictionary) when the index has none)."""
    ia, ib, _ = encode_chroms(query_col, index_col)
    icodes, ivalues = _chrom_values(index_col)
    shared_to_index = {}
    for row in range(len(ib)):
        shared_to_index[int(ib[row])] = int(icodes[row])
    return np.array([shared_to_index.get(int(c), len(ivalues)) for c in ia], np.int32)


def _lookup(index_col, query_col):
    icodes, ivalues = _chrom_values(index_col)
    qcodes, qvalues = _chrom_values(query_col)
    lut = _chrom_lookup(ivalues, qvalues)
    return lut[qcodes] if len(qvalues) else qcodes


STR = np.array(["chr1", "chr2", "chr10", "chrX"], dtype=object)


@pytest.mark.parametrize("index_col,query_col", [
    (STR, np.array(["chr2", "chrX", "chrUn", "chr1", "chr2"], dtype=object)),
    (np.array([0, 3, 7, 3], np.int32), np.array([7, 0, 1, 3], np.int64)),        # both integer: compared as integers
    (np.array(["0", "3", "7"], dtype=object), np.array([7, 0, 1, 3], np.int64)),   # int query, string index: as str
    (np.array([0, 3, 7], np.int64), np.array(["7", "0", "1", "03"], dtype=object)),  # string query, int index
    (np.array([1, 2], np.int32), np.zeros(0, np.int64)),
    (np.array(["1.5", "2"], dtype=object), np.array([1.5, 2.0, 2.5])),             # floats: as str, like the join
])
def test_lookup_matches_encode_chroms(index_col, query_col):
    got = _lookup(index_col, query_col)
    want = _lookup_like_encode_chroms(index_col, query_col)
    assert np.array_equal(got, want), (got, want)


def test_int_query_finds_string_chromosomes():
    got = _lookup(np.array(["1", "2", "3"], dtype=object), np.array([3, 1, 9], np.int64))
    assert got.tolist() == [2, 0, 3]


@pytest.mark.parametrize("col", [
    np.array(["chr1", None, "chr2"], dtype=object),
    np.array(["chr1", "chr2", None], dtype=object),          # (not only the first element is checked)
    np.array([1.0, float("nan")]),
])
def test_null_chroms_are_refused_like_the_ordinary_join(col):
    with pytest.raises(ValueError, match="NULL"):
        _chrom_values(col)
    with pytest.raises(ValueError, match="NULL"):
        encode_chroms(col, np.array(["chr1"], dtype=object))


def test_negative_integer_ids_are_refused_like_the_ordinary_join():
    with pytest.raises(ValueError, match="non-negative"):
        _chrom_lookup([0, 1], [-1, 1])
    with pytest.raises(ValueError, match="non-negative"):
        encode_chroms(np.array([-1, 1]), np.array([0, 1]))
    # an integer column beside a string one is compared as str: no error there, as in the ordinary join
    assert _chrom_lookup(["-1", "1"], [-1, 1]).tolist() == [0, 1]
