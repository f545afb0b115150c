"""The bytes ``giql_hip_index_info`` reports for a table index, pinned exactly at every step of its life: creation,
either preparation first, the other after it, each a second time -- needs a GPU.

The formulas are those of the arrays an index owns (``struct giql_hip_index``): 4 B per row and array, a
``1024 + n_chrom + 1`` word block of digit offsets and chromosome bounds, directories of ``2^(32 - wbits) + 1`` cells
(wbits = 16 .. 13), a rank per chromosome bound for NEAREST.  The directory over the start keys is shared by the two
preparations and counted once."""

import numpy as np
import pytest

from oracle import pyoracle as ora
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N, N_CHROM = 5_000, 3


@pytest.fixture(scope="module")
def eng():
    from giql_amd.engine import HipEngine

    e = HipEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def tables():
    r = np.random.default_rng(7)
    chrom = (np.arange(N) % N_CHROM).astype(np.int32)
    start = r.integers(0, 1_000_000, N).astype(np.int32)
    fixed = ora.Side(chrom, start, (start + 100).astype(np.int32))
    general = ora.Side(chrom, start, (start + r.integers(1, 901, N)).astype(np.int32))
    return {False: fixed, True: general}


def cells_of(grew):
    """the cells of one directory, from the 4 B each it added: 2^k + 1 with 16 <= k <= 19"""
    assert grew % 4 == 0, grew
    cells = grew // 4
    assert cells - 1 in (1 << 16, 1 << 17, 1 << 18, 1 << 19), cells
    return cells


@pytest.mark.parametrize("general", [False, True])
def test_index_info_bytes_are_the_arrays_the_index_owns(eng, tables, general):
    b = tables[general]
    created = 4 * N * (3 if general else 2) + 4 * (1024 + N_CHROM + 1)
    nearest_own = (8 * N if general else 0) + 4 * (N_CHROM + 1)    # without the shared directory

    index = eng.index_create(dev(b), N_CHROM)                      # the row operators' arrays first
    try:
        assert index.n == N and index.general == general
        assert index.nbytes == created
        index.prepare_rows()
        grew = index.nbytes - created
        if general:
            assert (grew - 4 * N) % 8 == 0, grew
            cells = cells_of((grew - 4 * N) // 2)                  # sorted end keys + two directories
        else:
            cells = cells_of(grew)                                 # one directory
        with_rows = index.nbytes
        index.prepare_rows()
        assert index.nbytes == with_rows
        index.prepare_nearest()
        assert index.nbytes == with_rows + nearest_own             # the directory was found there
        index.prepare_nearest()
        index.prepare_rows()
        assert index.nbytes == with_rows + nearest_own
    finally:
        index.close()

    index = eng.index_create(dev(b), N_CHROM)                      # NEAREST's arrays first
    try:
        assert index.nbytes == created
        index.prepare_nearest()
        assert index.nbytes == created + nearest_own + 4 * cells
        index.prepare_nearest()
        assert index.nbytes == created + nearest_own + 4 * cells
        index.prepare_rows()
        rows_own = 4 * N + 4 * cells if general else 0             # the shared directory is counted once
        assert index.nbytes == created + nearest_own + 4 * cells + rows_own
        assert index.nbytes == with_rows + nearest_own             # either order ends at the same sum
        index.prepare_rows()
        index.prepare_nearest()
        assert index.nbytes == with_rows + nearest_own
    finally:
        index.close()
