"""The row operators at and past their 32-bit limits, and execute() past 2^31 pairs and 2 GiB of strings -- needs a GPU.

Kernel level (through the C ABI, so that no engine-side slicing hides a limit): select at 0x7FFFFFF0 candidates with
and without id arrays, take_utf8 at exactly 2^31 - 1 gathered bytes, take / mark / segment_sum / pairs_checksum past
2^31 elements -- each against plain torch (or the C oracle for the checksum), compared on the device in chunks of
2^28 so that host memory stays small.  The limits themselves are pinned on both sides.

execute() level: tables built from clique blocks (every A row of a block overlaps every B row of it, blocks 1 Mb
apart), so that the exact answer of a residual join follows from per-block sorted scores with no oracle sweep.  The
INNER / SEMI / ANTI legs have more than 2^31 candidate pairs (HipEngine.select slices them), the string leg gathers
more than 2 GiB of names (execute splits the column into chunks that each fit int32 offsets).

Every test prints its wall time and the peak of torch's device allocations (the library's own workspace is not
counted there)."""

import ctypes
import time

import numpy as np
import pytest

from giql_amd import _lib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
pa = pytest.importorskip("pyarrow")
pc = pytest.importorskip("pyarrow.compute")

DEV = "cuda:0"
CHUNK = 1 << 28
SELECT_MAX = 0x7FFFFFF0        # giql_hip_select_expr_dev / giql_hip_take_utf8_plan_dev: most rows of one call
UTF8_MAX_BYTES = 0x7FFFFFFF


@pytest.fixture(scope="module")
def eng():
    from giql_amd.engine import HipEngine

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    e = HipEngine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _footprint(request):
    torch.zeros(1, device=DEV)          # (the allocator's statistics exist once the device is initialised)
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(DEV)
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize(DEV)
    print(f"\n[past_int32] {request.node.name}: {time.perf_counter() - t0:.1f} s, "
          f"peak torch HBM {torch.cuda.max_memory_allocated(DEV) / 2**30:.1f} GiB")
    torch.cuda.empty_cache()


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _chunks(n, size=CHUNK):
    for lo in range(0, n, size):
        yield lo, min(n, lo + size)


def _select_abi(e, preds, idx_a, idx_b, n, n_rows_a, n_rows_b, out_a, out_b):
    """One giql_hip_select_expr_dev call: (status, kept)."""
    c_preds, k, _keep, c_nodes, n_nodes = e._c_preds(preds)
    kept = ctypes.c_int64(-1)
    rc = e._L.giql_hip_select_expr_dev(e._h, c_preds, k, c_nodes if n_nodes else None, n_nodes, _ptr(idx_a), n_rows_a,
                                       _ptr(idx_b), n_rows_b, n, _ptr(out_a), _ptr(out_b), ctypes.byref(kept),
                                       e._stream())
    return rc, int(kept.value)


# ---------------------------------------------------------------------------------------------- select
def _residual(a_i32, b_i32, b_f64, b_valid):
    """a.x != b.x AND (a.x < 900 OR b.f > 50.0): keeps ~97 % of the candidates; b.f is NULL where b_valid is 0."""
    preds = [(("a", a_i32), "!=", ("b", b_i32)),
             (("a", a_i32), "<", ("lit", 900), 1), (("b", b_f64, b_valid), ">", ("lit", 50.0), 1)]

    def reference(ia, ib):
        x = a_i32[ia]
        return (x != b_i32[ib]) & ((x < 900) | ((b_f64[ib] > 50.0) & (b_valid[ib] != 0)))

    return preds, reference


def _columns(n_a, n_b, g):
    a_i32 = torch.randint(-1000, 1000, (n_a,), dtype=torch.int32, device=DEV, generator=g)
    b_i32 = torch.randint(-1000, 1000, (n_b,), dtype=torch.int32, device=DEV, generator=g)
    b_f64 = torch.rand(n_b, dtype=torch.float64, device=DEV, generator=g) * 100.0
    b_valid = (torch.rand(n_b, device=DEV, generator=g) < 0.97).to(torch.uint8)
    return a_i32, b_i32, b_f64, b_valid


def test_select_pairs_at_the_limit(eng):
    """0x7FFFFFF0 candidate pairs through id arrays: the kept pairs are the torch-evaluated predicate's survivors in
    input order (block offsets and output positions are u32 in k_select_scatter); one more candidate is refused."""
    g = _gen(31)
    n_a, n_b = 3_000_017, 5_000_011
    cols = _columns(n_a, n_b, g)
    preds, reference = _residual(*cols)
    # one spare element everywhere: the n + 1 call below is refused before it reads anything, and could not overrun
    idx_a = torch.randint(0, n_a, (SELECT_MAX + 1,), dtype=torch.int32, device=DEV, generator=g)
    idx_b = torch.randint(0, n_b, (SELECT_MAX + 1,), dtype=torch.int32, device=DEV, generator=g)
    idx_a[SELECT_MAX - 1], idx_b[SELECT_MAX - 1] = n_a - 1, n_b - 1
    out_a = torch.full((SELECT_MAX + 1,), -7, dtype=torch.int32, device=DEV)
    out_b = torch.full((SELECT_MAX + 1,), -7, dtype=torch.int32, device=DEV)

    rc, kept = _select_abi(eng, preds, idx_a, idx_b, SELECT_MAX + 1, n_a, n_b, out_a, out_b)
    assert rc == _lib.GIQL_ERR_INVALID
    assert int(out_a[0]) == -7 and int(out_b[-1]) == -7

    rc, kept = _select_abi(eng, preds, idx_a, idx_b, SELECT_MAX, n_a, n_b, out_a, out_b)
    assert rc == _lib.GIQL_OK
    pos = 0
    for lo, hi in _chunks(SELECT_MAX):
        ia, ib = idx_a[lo:hi], idx_b[lo:hi]
        m = reference(ia.long(), ib.long())
        c = int(m.sum())
        assert torch.equal(out_a[pos:pos + c], ia[m]) and torch.equal(out_b[pos:pos + c], ib[m]), lo
        pos += c
        del ia, ib, m
    assert kept == pos and 0.9 * SELECT_MAX < kept < SELECT_MAX
    assert int(out_a[kept]) == -7        # nothing written past the kept count


def test_select_row_ids_at_the_limit(eng):
    """0x7FFFFFF0 candidates WITHOUT id arrays: candidate i addresses row i of both sides ((int)i in the kernel)
    and is written as its own id."""
    g = _gen(32)
    n = SELECT_MAX
    cols = _columns(n, n, g)
    preds, reference = _residual(*cols)
    out_a = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    out_b = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    rc, kept = _select_abi(eng, preds, None, None, n, n, n, out_a, out_b)
    assert rc == _lib.GIQL_OK
    pos = 0
    for lo, hi in _chunks(n):
        r = torch.arange(lo, hi, dtype=torch.int64, device=DEV)
        want = torch.nonzero(reference(r, r)).flatten().add_(lo).to(torch.int32)
        c = int(want.shape[0])
        assert torch.equal(out_a[pos:pos + c], want) and torch.equal(out_b[pos:pos + c], want), lo
        pos += c
        del r, want
    assert kept == pos and 0.9 * n < kept < n
    if kept < n:
        assert int(out_a[kept]) == -7


def test_engine_select_slices_give_one_stable_filter(eng, monkeypatch):
    """HipEngine.select with small slices (the production slice is 2^30): pairs, row ids, one wanted side, a
    one-sided predicate over a side addressed by the candidate index, and an empty input -- all equal to one call."""
    from giql_amd.engine import HipEngine

    g = _gen(33)
    n = 100_003
    cols = _columns(n, n, g)
    preds, reference = _residual(*cols)
    idx_a = torch.randint(0, n, (n,), dtype=torch.int32, device=DEV, generator=g)
    idx_b = torch.randint(0, n, (n,), dtype=torch.int32, device=DEV, generator=g)
    one_sided = [(("a", cols[0]), ">", ("lit", -500))]
    cases = [dict(preds=preds, idx_a=idx_a, idx_b=idx_b, n_rows_a=n, n_rows_b=n),
             dict(preds=preds, n=n, n_rows_a=n, n_rows_b=n),
             dict(preds=preds, idx_a=idx_a, idx_b=idx_b, n_rows_a=n, n_rows_b=n, want=("b",)),
             dict(preds=one_sided, n=n, n_rows_a=n, want=("a",)),
             dict(preds=one_sided, n=n, n_rows_a=n),
             dict(preds=preds, idx_a=idx_a[:0], idx_b=idx_b[:0], n_rows_a=n, n_rows_b=n)]
    whole = [eng.select(**c) for c in cases]
    r = torch.arange(n, device=DEV)
    assert torch.equal(whole[0][0], idx_a[reference(idx_a.long(), idx_b.long())])
    assert torch.equal(whole[1][0].long(), torch.nonzero(reference(r, r)).flatten())
    assert torch.equal(whole[4][1].long(), torch.nonzero(cols[0] > -500).flatten())
    for size in (1 << 30, 4096, 2048 * 7 + 13, 997):
        monkeypatch.setattr(HipEngine, "SELECT_SLICE", size)
        for c, w in zip(cases, whole):
            got = eng.select(**c)
            for x, y in zip(got, w):
                assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), (size, c.keys())
    # a side addressed by the candidate index is still checked against its row count in every slice
    monkeypatch.setattr(HipEngine, "SELECT_SLICE", 4096)
    with pytest.raises(_lib.GiqlHipError):
        eng.select(one_sided, n=n, n_rows_a=n - 1, want=("a",))


# ------------------------------------------------------------------------------------------ take_utf8
def _utf8_source(seed):
    """A source column whose rows have lengths that are not multiples of 4 and start at unaligned offsets, and a
    gather of exactly 2^31 - 1 bytes: one row of more than 1 MiB, ~65 KiB rows, short rows of either copy path
    (<= 32 bytes per lane, longer per wave), empty rows and idx = -1, and a remainder row last.  Returns
    (offsets, idx, idx_over, src_len, data_bytes): idx_over gathers one byte more."""
    r = np.random.default_rng(seed)
    lens = [np.array([1_048_583], np.int64),                                    # > 1 MiB, whole-wave path
            65536 + r.choice(np.array([-3, -2, -1, 1, 2, 3]), 4096),            # ~65 KiB
            r.integers(0, 41, 4096),                                            # 0..40 bytes
            r.integers(33, 301, 2048)]
    lens = np.concatenate(lens).astype(np.int64)
    k_long, k_short = 1 + np.arange(4096), 4097 + np.arange(4096)
    k_mid = 8193 + np.arange(2048)
    kind = r.random(200_000)
    cand = np.where(kind < 0.25, r.choice(k_long, kind.shape[0]),
                    np.where(kind < 0.85, r.choice(k_short, kind.shape[0]),
                             np.where(kind < 0.95, r.choice(k_mid, kind.shape[0]), -1)))
    cand[:3] = [0, -1, 1]
    glen = np.where(cand >= 0, lens[np.maximum(cand, 0)], 0)
    target = UTF8_MAX_BYTES
    csum = np.cumsum(glen)
    p = int(np.searchsorted(csum, target - 1, side="right"))      # the longest prefix with room for >= 1 byte
    rem = target - int(csum[p - 1])
    assert 1 <= rem <= 65539 and p < cand.shape[0]
    n_src = lens.shape[0]
    lens = np.concatenate([lens, [rem, rem + 1]])
    idx = np.concatenate([cand[:p], [n_src]]).astype(np.int32)
    idx_over = idx.copy()
    idx_over[-1] = n_src + 1
    offsets = np.concatenate([[3], 3 + np.cumsum(lens)]).astype(np.int64)    # 3 junk bytes in front: unaligned
    assert offsets[-1] < 2**31
    return offsets.astype(np.int32), idx, idx_over, lens, int(offsets[-1])


def test_take_utf8_at_exactly_int32_max_bytes(eng):
    g = _gen(41)
    off, idx, idx_over, lens, n_data = _utf8_source(41)
    off_d = torch.from_numpy(off).to(DEV)
    data = torch.randint(0, 256, (n_data,), dtype=torch.uint8, device=DEV, generator=g)
    idx_d = torch.from_numpy(idx).to(DEV)
    n = int(idx.shape[0])
    assert n > 100_000 and (idx < 0).sum() > 1000

    # one byte more: GIQL_ERR_CAPACITY, no byte count, nothing to fill
    over_d = torch.from_numpy(idx_over).to(DEV)
    out_off = torch.empty(n + 1, dtype=torch.int32, device=DEV)
    nb = ctypes.c_int64(-1)
    rc = eng._L.giql_hip_take_utf8_plan_dev(eng._h, off_d.data_ptr(), off.shape[0] - 1, over_d.data_ptr(), n,
                                            out_off.data_ptr(), ctypes.byref(nb), eng._stream())
    assert rc == _lib.GIQL_ERR_CAPACITY and nb.value == 0
    with pytest.raises(_lib.GiqlHipError, match="exceeds int32 offsets"):
        eng.take_utf8(off_d, data, over_d)
    del over_d, out_off

    o_got, d_got = eng.take_utf8(off_d, data, idx_d)
    assert int(o_got[-1]) == UTF8_MAX_BYTES and int(d_got.shape[0]) == UTF8_MAX_BYTES
    glen = torch.where(idx_d >= 0, torch.from_numpy(lens).to(DEV)[idx_d.clamp(min=0).long()], 0)
    want_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), torch.cumsum(glen, 0)])
    assert torch.equal(o_got.long(), want_off)
    # every output byte against the source byte it comes from
    src_start = off_d.long()[idx_d.clamp(min=0).long()]
    ends = want_off[1:].contiguous()
    for lo, hi in _chunks(UTF8_MAX_BYTES):
        p = torch.arange(lo, hi, dtype=torch.int64, device=DEV)
        row = torch.searchsorted(ends, p, right=True)
        src = src_start[row] + (p - want_off[row])
        assert torch.equal(d_got[lo:hi], data[src]), lo
        del p, row, src
    # (and spelt out on the host: the > 1 MiB row, the row after it and the remainder row in full)
    o_h = o_got.cpu().numpy().astype(np.int64)
    for i in (0, 2, n - 1):
        s = int(off[idx[i]])
        assert np.array_equal(d_got[o_h[i]:o_h[i + 1]].cpu().numpy(), data[s:s + int(lens[idx[i]])].cpu().numpy()), i
    assert o_h[1] == o_h[2]                  # idx = -1: an empty value


# ----------------------------------------------------------------------------------------------- take
def test_take_fixed_width_past_2_pow_31_rows(eng):
    """2^31 + 5 ids over 1-, 4-, 8- and 16-byte columns against torch.index_select; idx < 0 at the head, the tail
    (the scalar remainder after the 4-row vectors) and across 4-row vector boundaries gives zero bytes."""
    g = _gen(51)
    n, n_rows = 2**31 + 5, (1 << 20) + 3
    idx = torch.randint(0, n_rows, (n,), dtype=torch.int32, device=DEV, generator=g)
    neg = [0, 1, 3, 4, 7, 8, 2**31 - 4, 2**31 - 1, 2**31, 2**31 + 3, n - 2, n - 1]
    idx[torch.tensor(neg, device=DEV)] = -1
    idx[5], idx[2**31 + 1] = n_rows - 1, n_rows - 1
    u8 = torch.randint(0, 256, (n_rows,), dtype=torch.uint8, device=DEV, generator=g)
    i32 = torch.randint(-2**31, 2**31 - 1, (n_rows,), dtype=torch.int32, device=DEV, generator=g)
    i64 = torch.randint(-2**62, 2**62, (n_rows,), dtype=torch.int64, device=DEV, generator=g)
    c128 = torch.complex(torch.rand(n_rows, dtype=torch.float64, device=DEV, generator=g),
                         torch.rand(n_rows, dtype=torch.float64, device=DEV, generator=g))
    cols = [u8, i32, i64, c128]
    assert [c.element_size() for c in cols] == [1, 4, 8, 16]
    outs = eng.take(cols, idx)
    for lo, hi in _chunks(n):
        ix = idx[lo:hi]
        bad = ix < 0
        safe = ix.clamp(min=0).long()
        for c, o in zip(cols, outs):
            want = c.index_select(0, safe)
            want[bad] = 0
            assert torch.equal(o[lo:hi], want), (lo, c.dtype)
            del want
        del ix, bad, safe
    assert all(int(o[-1].abs()) == 0 for o in outs[:3]) and int(outs[0][5]) == int(u8[-1])


# ------------------------------------------------------------------------- mark, segment_sum, checksum
def test_mark_past_2_pow_31_ids(eng):
    g = _gen(61)
    n, n_rows = 2**31 + 7, 0x7FFFFFFF
    idx = torch.randint(0, n_rows, (n,), dtype=torch.int32, device=DEV, generator=g)
    idx[-1] = n_rows - 1
    idx[2**31] = 0
    flags = eng.mark(idx, n_rows)
    want = torch.zeros(n_rows, dtype=torch.uint8, device=DEV)
    for lo, hi in _chunks(n):
        want.index_fill_(0, idx[lo:hi].long(), 1)
    assert torch.equal(flags, want) and int(flags[-1]) == 1 and int(flags[0]) == 1


def test_segment_sum_past_2_pow_31_rows(eng):
    """int64 values near +-2^62 (a sum that wrapped or was cut to 32 bits shows); the last group only gets rows
    past 2^31."""
    g = _gen(62)
    n, n_groups = 2**31 + 3, 65_537
    values = torch.randint(-2**62, 2**62, (n,), dtype=torch.int64, device=DEV, generator=g)
    groups = torch.randint(0, n_groups - 1, (n,), dtype=torch.int32, device=DEV, generator=g)
    groups[2**31:] = n_groups - 1
    values[-1] = 2**62 + 12345
    sums = torch.empty(n_groups, dtype=torch.int64, device=DEV)
    _lib.check(eng._L.giql_hip_segment_sum_dev(eng._h, values.data_ptr(), groups.data_ptr(), n, sums.data_ptr(),
                                               n_groups, eng._stream()))
    want = torch.zeros(n_groups, dtype=torch.int64, device=DEV)
    for lo, hi in _chunks(n):
        want.index_add_(0, groups[lo:hi].long(), values[lo:hi])
    assert torch.equal(sums, want)
    assert int(sums[-1]) == int(values[2**31:].sum())


def test_pairs_checksum_past_2_pow_31_pairs(eng):
    """The checksum is a sum mod 2^64 over the pairs (ora_pairs_checksum in oracle/giql_oracle.c), so the oracle's
    value over chunks adds up to the whole; the device's must equal it."""
    from oracle import pyoracle as ora

    g = _gen(63)
    n = 2**31 + 9
    ra = torch.randint(-2**31, 2**31 - 1, (n,), dtype=torch.int32, device=DEV, generator=g)
    rb = torch.randint(-2**31, 2**31 - 1, (n,), dtype=torch.int32, device=DEV, generator=g)
    want = 0
    for lo, hi in _chunks(n):
        want = (want + ora.c_pairs_checksum(ra[lo:hi].cpu().numpy(), rb[lo:hi].cpu().numpy())) % 2**64
    got = eng.pairs_checksum(ra, rb)
    assert got == want
    assert (eng.pairs_checksum(ra[:2**31], rb[:2**31]) + eng.pairs_checksum(ra[2**31:], rb[2**31:])) % 2**64 == got


# --------------------------------------------------------------------------------- execute() past 2^31
def _clique_tables(seed, n_chrom, n_blocks, lo, hi):
    """Two tables of clique blocks: chromosome c holds n_blocks blocks 1 Mb apart; in a block every row starts in
    [0, 500) and ends in [500, 1000), so every A row of a block overlaps every B row of it and nothing else.  Rows are
    shuffled; each has a random int32 score with ties.  Returns ({name: arrays}, block of each row) per side."""
    r = np.random.default_rng(seed)
    n_blk = n_chrom * n_blocks
    names = pa.array([f"chr{c + 1}" for c in range(n_chrom)])
    sides = []
    for _ in range(2):
        sizes = r.integers(lo, hi + 1, n_blk)
        block = np.repeat(np.arange(n_blk, dtype=np.int64), sizes)
        block = block[r.permutation(block.shape[0])]
        base = (block % n_blocks) * 1_000_000 + 10_000
        cols = {"chrom": pc.take(names, pa.array(block // n_blocks)),
                "start": (base + r.integers(0, 500, block.shape[0])).astype(np.int32),
                "end": (base + r.integers(500, 1000, block.shape[0])).astype(np.int32),
                "score": r.integers(0, 3000, block.shape[0]).astype(np.int32)}
        sides.append((cols, block, np.bincount(block, minlength=n_blk)))
    return sides


def _kept_per_a_row(sa, sb):
    """For every A row: how many B rows of its block have a greater score, and the sum of their scores
    (per block, the B scores sorted once; searchsorted gives each answer)."""
    (ca, blk_a, _), (cb, blk_b, _) = sa, sb
    key_b = blk_b * 2**32 + cb["score"]
    order = np.argsort(key_b, kind="stable")
    key_b = key_b[order]
    csum = np.concatenate([[0], np.cumsum(cb["score"][order].astype(np.int64))])
    first = np.searchsorted(key_b, blk_a * 2**32 + ca["score"], side="right")
    end = np.searchsorted(key_b, (blk_a + 1) * 2**32, side="left")
    return end - first, csum[end] - csum[first]


def _cliques():
    sa, sb = _clique_tables(71, 24, 40, 1300, 1800)
    n_pairs = int((sa[2] * sb[2]).sum())
    assert 2.2e9 < n_pairs < 2.45e9 and max(sa[2].max(), sb[2].max()) < 4096
    cnt, ssum = _kept_per_a_row(sa, sb)
    t = {"ta": pa.table(sa[0]), "tb": pa.table(sb[0])}
    return t, sa, sb, n_pairs, cnt, ssum


@pytest.fixture(scope="module")
def cliques():
    return _cliques()


Q_RESIDUAL = ("SELECT {cols} FROM ta a {kind} JOIN tb b ON a.interval INTERSECTS b.interval AND a.score < b.score")


def test_execute_inner_residual_past_2_pow_31_candidates(eng, cliques):
    from giql_amd.execute import execute
    from giql_amd.transpile import transpile

    t, sa, sb, n_pairs, cnt, ssum = cliques
    n_a, n_b = sa[1].shape[0], sb[1].shape[0]
    plan = transpile(Q_RESIDUAL.format(cols="b.score AS s", kind=""), tables=["ta", "tb"], dialect="hip")
    ra, rb = execute(plan, t, engine=eng, return_indices=True)
    n_kept = int(cnt.sum())
    assert 2**30 < n_kept < n_pairs and ra.shape[0] == n_kept == rb.shape[0]
    assert int(ra.min()) >= 0 and int(ra.max()) < n_a and int(rb.min()) >= 0 and int(rb.max()) < n_b
    mult = torch.zeros(n_a, dtype=torch.int64, device=DEV)
    for lo, hi in _chunks(n_kept):
        mult += torch.bincount(torch.from_numpy(ra[lo:hi]).to(DEV), minlength=n_a)
    assert torch.equal(mult.cpu(), torch.from_numpy(cnt.astype(np.int64)))
    s = slice(None, None, 997)
    pa_, pb_ = ra[s], rb[s]
    assert (sa[0]["score"][pa_] < sb[0]["score"][pb_]).all() and np.array_equal(sa[1][pa_], sb[1][pb_])
    del ra, rb, pa_, pb_, mult
    torch.cuda.empty_cache()

    out = execute(plan, t, engine=eng)
    assert out.num_rows == n_kept
    assert pc.sum(out.column("s")).as_py() == int(ssum.sum())


@pytest.mark.parametrize("kind", ["SEMI", "ANTI"])
def test_execute_semi_anti_residual_past_2_pow_31_candidates(eng, cliques, kind):
    """An A row has a pair that passes exactly when its block's largest B score is greater than its own."""
    from giql_amd.execute import execute
    from giql_amd.transpile import transpile

    t, sa, sb, n_pairs, cnt, ssum = cliques
    plan = transpile(Q_RESIDUAL.format(cols="a.start", kind=kind), tables=["ta", "tb"], dialect="hip")
    rows = execute(plan, t, engine=eng, return_indices=True)
    want = np.nonzero((cnt > 0) if kind == "SEMI" else (cnt == 0))[0]
    assert 0 < want.shape[0] < sa[1].shape[0]
    assert np.array_equal(np.asarray(rows, np.int64), want)


def _names(r, n):
    """n random lowercase names of 12-20 bytes, 5 % NULL (whose slots keep their bytes, as Arrow allows)."""
    lens = r.integers(12, 21, n)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    data = r.integers(97, 123, int(offsets[-1])).astype(np.uint8)
    valid = r.random(n) >= 0.05
    vbuf = pa.py_buffer(np.packbits(valid, bitorder="little").tobytes())
    arr = pa.Array.from_buffers(pa.string(), n, [vbuf, pa.py_buffer(offsets), pa.py_buffer(data)],
                                null_count=int((~valid).sum()))
    return arr, lens, valid


def _take_rows(col, rows):
    """``col[rows]`` chunk by chunk (pyarrow's take concatenates the chunks first, which 2 GiB of strings overflow)."""
    bounds = np.cumsum([0] + [len(c) for c in col.chunks])
    which = np.searchsorted(bounds, rows, side="right") - 1
    order = np.argsort(which, kind="stable")
    parts = [col.chunk(k).take(pa.array(rows[order][which[order] == k] - bounds[k])) for k in range(col.num_chunks)]
    return pa.concat_arrays(parts).take(pa.array(np.argsort(order)))


def test_execute_projects_names_past_2_gib(eng):
    """~1.5e8 pairs projecting b.name (12-20 bytes, some NULL) from a sliced table: more than 2^31 bytes in all,
    returned as string chunks that each fit int32 offsets.  Pair order is unspecified, so every checked row is
    matched through b.bid (a unique row number projected beside it): name == take(source name, bid)."""
    from giql_amd.execute import execute
    from giql_amd.transpile import transpile

    sa, sb = _clique_tables(72, 24, 40, 350, 450)
    n_pairs = int((sa[2] * sb[2]).sum())
    assert 1.4e8 < n_pairs < 1.8e8
    r = np.random.default_rng(72)
    pad = 7
    n_b = sb[1].shape[0]
    names, lens, valid = _names(r, n_b + pad)
    cols_b = {k: (pa.concat_arrays([pa.array(v[:pad]), pa.array(v)]) if not isinstance(v, pa.Array)
                  else pa.concat_arrays([v.slice(0, pad), v])) for k, v in sb[0].items()}
    cols_b["name"] = names
    cols_b["bid"] = pa.array(np.arange(-pad, n_b, dtype=np.int32))
    tb = pa.table(cols_b).slice(pad)
    src_name = tb.column("name").chunk(0)
    assert src_name.offset == pad and tb.column("bid").chunk(0).offset == pad
    lens, valid = lens[pad:], valid[pad:]
    per_b = sa[2][sb[1]]                      # A rows in each B row's block = that row's pair count
    want_bytes = int((per_b * lens).sum())
    assert want_bytes > 2**31 + 2**27

    plan = transpile("SELECT b.name AS name, b.bid AS bid FROM ta a JOIN tb b ON a.interval INTERSECTS b.interval",
                     tables=["ta", "tb"], dialect="hip")
    out = execute(plan, {"ta": pa.table(sa[0]), "tb": tb}, engine=eng)
    assert out.num_rows == n_pairs
    name, bid = out.column("name"), out.column("bid")
    assert name.type == pa.string() and name.num_chunks >= 2
    sizes = [c.buffers()[2].size for c in name.chunks]
    assert all(s < 2**31 for s in sizes) and sum(sizes) == want_bytes
    assert name.null_count == int(per_b[~valid].sum())
    assert int(pc.sum(pc.binary_length(name)).as_py()) == int((per_b * lens)[valid].sum())
    # rows at every chunk boundary, and a seeded sample of 1M rows
    bounds = np.cumsum([0] + [len(c) for c in name.chunks])
    edge = np.unique(np.clip(np.concatenate([bounds - 2, bounds - 1, bounds, bounds + 1]), 0, n_pairs - 1))
    sample = np.unique(np.concatenate([edge, np.random.default_rng(73).integers(0, n_pairs, 1_000_000)]))
    got, ids = _take_rows(name, sample), _take_rows(bid, sample)
    assert ids.null_count == 0 and pc.min(ids).as_py() >= 0 and pc.max(ids).as_py() < n_b
    assert got.equals(pc.take(src_name, ids))


@pytest.mark.parametrize("max_bytes,max_rows", [(2000, 10**9), (10**9, 333), (997, 50)])
def test_execute_splits_names_at_small_limits(eng, monkeypatch, max_bytes, max_rows):
    """The same row split at limits small enough to run in milliseconds: the chunks of the column's own type hold the
    rows of the unsplit projection, NULLs and a sliced source column included."""
    from giql_amd import execute as ex
    from giql_amd.transpile import transpile

    sa, sb = _clique_tables(74, 2, 3, 20, 30)
    r = np.random.default_rng(74)
    names, _lens, _valid = _names(r, sb[1].shape[0] + 3)
    tb = pa.table({**{k: pa.array(np.concatenate([v[:3], v])) if not isinstance(v, pa.Array)
                      else pa.concat_arrays([v.slice(0, 3), v]) for k, v in sb[0].items()},
                   "name": names, "bid": pa.array(np.arange(-3, sb[1].shape[0], dtype=np.int32))}).slice(3)
    tables = {"ta": pa.table(sa[0]), "tb": tb.cast(tb.schema.set(tb.schema.get_field_index("name"),
                                                                  pa.field("name", pa.binary())))}
    plan = transpile("SELECT b.name AS name, b.bid AS bid FROM ta a JOIN tb b ON a.interval INTERSECTS b.interval",
                     tables=["ta", "tb"], dialect="hip")
    whole = ex.execute(plan, tables, engine=eng)
    monkeypatch.setattr(ex, "UTF8_MAX_BYTES", max_bytes)
    monkeypatch.setattr(ex, "UTF8_MAX_ROWS", max_rows)
    split = ex.execute(plan, tables, engine=eng)
    name = split.column("name")
    assert name.type == pa.binary() and name.num_chunks > 2 and whole.column("name").num_chunks == 1
    assert all(len(c) <= max_rows and c.buffers()[2].size <= max_bytes for c in name.chunks)
    rows = lambda t: sorted(zip(t.column("bid").to_pylist(), t.column("name").to_pylist()), key=lambda x: (x[0], x[1] or b""))
    assert rows(split) == rows(whole) and split.column("name").null_count == whole.column("name").null_count > 0
    src = tables["tb"].column("name").chunk(0)
    assert all(n == src[b].as_py() for b, n in rows(split)[::7])
