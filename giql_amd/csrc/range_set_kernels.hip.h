// range_set_kernels.hip.h -- `interval <op> ANY('chr:lo-hi', ...)` over one table (giql_hip_range_set_any_dev).
//
// The predicate is an OR of K three-term conjunctions; as residuals of the select kernel its normal form has 3^K
// clauses.  Here a block stages one set's table (range_set_prepare.h: the ranges ordered by (chromosome, one bound),
// beside a running maximum / minimum of the other bound that restarts at every chromosome; 28 bytes per range, 28 KB
// at the cap) in LDS once and walks tiles of RSET_TILE rows: every thread reads four consecutive rows of the three
// int32 columns in 16-byte loads, answers each with ONE binary search over (chromosome, bound) -- log2 K steps in
// LDS -- and one compare with the aggregate, and writes the four answers as one 32-bit store per output array.  The
// columns are read as they lie in memory: the table's coordinate encoding was moved onto the int64 bounds by the
// caller, nothing is added to a row's value, so nothing wraps.  There is no linearised axis, hence no span limit.
//
// Output per set: a three-valued result as two byte arrays, `value` (1 = TRUE) and `valid` (0 = SQL NULL, value 0):
// the shape of a select operand of type u8 with its validity.  A row with a NULL among chrom / start / end takes the
// plain loop over the K ranges in three-valued logic (rs_row_nulls); such rows are rare.  A row whose chromosome no
// range names -- a code outside the dictionary included -- is FALSE.
#pragma once
#include "dev_common.hip.h"
#include "range_set_prepare.h"

namespace giql {

constexpr int RSET_NT = 256;
constexpr int RSET_VEC = 4;                          // rows per thread and tile (one 16-byte load per column)
constexpr u32 RSET_TILE = (u32)RSET_NT * RSET_VEC;       // rows per tile
typedef int rs_i4 __attribute__((ext_vector_type(4)));

struct RsSetDev {
  const int32_t* chrom;   // device: the set's table, k entries each
  const i64* key;
  const i64* other;
  const i64* agg;
  int32_t k, op;
  uint8_t* value;         // device outputs, n bytes each
  uint8_t* valid;
};

struct RsArgs {
  RsSetDev set[RSET_MAX_SETS];
};

// One row whose three fields are all known: 1 = some range matches.
__device__ __forceinline__ u32 rs_row(int op, int k, const int32_t* s_chrom, const i64* s_key, const i64* s_agg,
                                      int32_t c, i64 start, i64 end) {
  const i64 probe = op == RSET_INTERSECTS ? end : start;
  int lo = 0, hi = k;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const int32_t mc = s_chrom[mid];
    const i64 mk = s_key[mid];
    const bool below = mc < c || (mc == c && (op == RSET_WITHIN ? mk <= probe : mk < probe));
    if (below)
      lo = mid + 1;
    else
      hi = mid;
  }
  if (op == RSET_CONTAINS) return (lo < k && s_chrom[lo] == c && s_agg[lo] <= end) ? 1u : 0u;
  if (lo == 0 || s_chrom[lo - 1] != c) return 0u;
  return (op == RSET_INTERSECTS ? s_agg[lo - 1] > start : s_agg[lo - 1] >= end) ? 1u : 0u;
}

// One row with a NULL among its fields: the OR over the K terms in SQL's three-valued logic.  A term is FALSE when a
// known conjunct is false, else NULL when a conjunct is unknown, else TRUE.  Returns value | valid << 8.
__device__ __noinline__ u32 rs_row_nulls(int op, int k, const int32_t* s_chrom, const i64* s_key, const i64* s_other,
                                         int32_t c, i64 start, i64 end, bool ok_c, bool ok_s, bool ok_e) {
  bool any_true = false, any_null = false;
  for (int j = 0; j < k; j++) {
    const i64 on_start = op == RSET_INTERSECTS ? s_other[j] : s_key[j];
    const i64 on_end = op == RSET_INTERSECTS ? s_key[j] : s_other[j];
    bool pass_s, pass_e;
    if (op == RSET_INTERSECTS) {
      pass_s = start < on_start;
      pass_e = end > on_end;
    } else if (op == RSET_CONTAINS) {
      pass_s = start <= on_start;
      pass_e = end >= on_end;
    } else {
      pass_s = start >= on_start;
      pass_e = end <= on_end;
    }
    const bool is_false = (ok_c && s_chrom[j] != c) || (ok_s && !pass_s) || (ok_e && !pass_e);
    if (is_false) continue;
    if (ok_c && ok_s && ok_e)
      any_true = true;
    else
      any_null = true;
  }
  const u32 valid = (any_true || !any_null) ? 1u : 0u;
  return (any_true ? 1u : 0u) | (valid << 8);
}

// grid = (blocks, sets).  vec_ok: the three columns are 16-byte aligned and every validity / output array 4-byte
// aligned (the host checks); without it every row goes through the scalar tail.
__global__ __launch_bounds__(RSET_NT) void k_range_set_any(const int32_t* __restrict__ chrom,
                                                         const int32_t* __restrict__ start,
                                                         const int32_t* __restrict__ end,
                                                         const uint8_t* __restrict__ v_chrom,
                                                         const uint8_t* __restrict__ v_start,
                                                         const uint8_t* __restrict__ v_end, u64 n, RsArgs args,
                                                         int vec_ok) {
  __shared__ int32_t s_chrom[RSET_MAX_RANGES];
  __shared__ i64 s_key[RSET_MAX_RANGES];
  __shared__ i64 s_other[RSET_MAX_RANGES];
  __shared__ i64 s_agg[RSET_MAX_RANGES];
  const RsSetDev S = args.set[blockIdx.y];
  const int k = S.k < RSET_MAX_RANGES ? S.k : RSET_MAX_RANGES;
  const int op = S.op;
  for (int i = threadIdx.x; i < k; i += RSET_NT) {
    s_chrom[i] = S.chrom[i];
    s_key[i] = S.key[i];
    s_other[i] = S.other[i];
    s_agg[i] = S.agg[i];
  }
  __syncthreads();
  const bool nulls = v_chrom || v_start || v_end;
  const u64 n_tiles = (n + RSET_TILE - 1) / RSET_TILE;
  for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const u64 base = t * RSET_TILE + (u64)threadIdx.x * RSET_VEC;
    if (base >= n) continue;
    int32_t c[RSET_VEC], s[RSET_VEC], e[RSET_VEC];
    u32 okc = 0x01010101u, oks = 0x01010101u, oke = 0x01010101u;  // a validity byte per row
    const bool full = vec_ok && base + RSET_VEC <= n;
    if (full) {
      const rs_i4 vc = ld_stream(reinterpret_cast<const rs_i4*>(chrom + base));
      const rs_i4 vs = ld_stream(reinterpret_cast<const rs_i4*>(start + base));
      const rs_i4 ve = ld_stream(reinterpret_cast<const rs_i4*>(end + base));
      c[0] = vc.x, c[1] = vc.y, c[2] = vc.z, c[3] = vc.w;
      s[0] = vs.x, s[1] = vs.y, s[2] = vs.z, s[3] = vs.w;
      e[0] = ve.x, e[1] = ve.y, e[2] = ve.z, e[3] = ve.w;
      if (v_chrom) okc = *reinterpret_cast<const u32*>(v_chrom + base);
      if (v_start) oks = *reinterpret_cast<const u32*>(v_start + base);
      if (v_end) oke = *reinterpret_cast<const u32*>(v_end + base);
    } else {
      okc = oks = oke = 0;
#pragma unroll
      for (int j = 0; j < RSET_VEC; j++) {
        const u64 r = base + j;
        const bool in = r < n;
        c[j] = in ? chrom[r] : 0;
        s[j] = in ? start[r] : 0;
        e[j] = in ? end[r] : 0;
        okc |= (u32)(in && (!v_chrom || v_chrom[r]) ? 1 : 0) << (8 * j);
        oks |= (u32)(in && (!v_start || v_start[r]) ? 1 : 0) << (8 * j);
        oke |= (u32)(in && (!v_end || v_end[r]) ? 1 : 0) << (8 * j);
      }
    }
    u32 value = 0, valid = 0;
#pragma unroll
    for (int j = 0; j < RSET_VEC; j++) {
      const bool kc = (okc >> (8 * j)) & 0xFFu, ks = (oks >> (8 * j)) & 0xFFu, ke = (oke >> (8 * j)) & 0xFFu;
      u32 vv;   // value | valid << 8 (in the scalar tail the rows past the table's end are computed and not stored)
      if (!nulls || (kc && ks && ke))
        vv = rs_row(op, k, s_chrom, s_key, s_agg, c[j], (i64)s[j], (i64)e[j]) | 0x100u;
      else
        vv = rs_row_nulls(op, k, s_chrom, s_key, s_other, c[j], (i64)s[j], (i64)e[j], kc, ks, ke);
      value |= (vv & 1u) << (8 * j);
      valid |= ((vv >> 8) & 1u) << (8 * j);
    }
    if (full) {
      *reinterpret_cast<u32*>(S.value + base) = value;
      *reinterpret_cast<u32*>(S.valid + base) = valid;
    } else {
#pragma unroll
      for (int j = 0; j < RSET_VEC; j++) {
        if (base + j < n) {
          S.value[base + j] = (uint8_t)((value >> (8 * j)) & 0xFFu);
          S.valid[base + j] = (uint8_t)((valid >> (8 * j)) & 0xFFu);
        }
      }
    }
  }
}

}  // namespace giql
