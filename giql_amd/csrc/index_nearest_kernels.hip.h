// giql_amd/csrc/index_nearest_kernels.hip.h -- NEAREST (k = 1, unstranded) against a table INDEX.
//
// The logic is k_nearest's (aux_kernels.hip.h; the distance CASE of _distance.py:67-87, the order ABS(d), start, end
// of nearest.py:392), read off an index instead of two freshly sorted sides: one thread per query row in INPUT
// order, the row's ranks found through the directory of bucket boundaries (ir_rank2, index_rows_kernels.hip.h), the
// result written at the row's own index -- two coalesced stores, no record array, no unpack pass, no scatter.
//
// A query row keeps its canonical coordinates as 64-bit chromosome-local values.  Its KEYS on the index's axis are
// clamped by the rules of ir_place (start at 0, end at the chromosome's first[c + 1]) and serve ONLY to find ranks,
// which are clamped to the chromosome's own rows [chrom_lo[c], chrom_lo[c + 1]); every distance comes from the
// unclamped coordinates and the target's local ones (key[j] - first[c]).  So a row below 0, beyond the indexed range
// or reaching over either end still gets its nearest target on the chromosome and its true distance.
//
// Fixed-length form (length L): the prefix max of the ends is key + L.  With hi = #{key < a.end} and
// lo = #{key < a.start - L + 1} -- two independent directory searches -- the rows [lo, hi) are exactly the
// overlapping ones; with none, the nearest upstream end is key[hi - 1] + L and its first row the head of that key's
// run, the nearest downstream row is row hi.
// General form: nr_pmax[n] = prefix max of the end keys in (start, end) order and nr_rid[n] = the row ids in that
// order (giql_hip_index_prepare_nearest_dev), searched backwards from hi by the gallop helpers.
#pragma once

#include "aux_kernels.hip.h"
#include "index_rows_kernels.hip.h"

namespace giql {

// What the NEAREST kernel reads of an index (all device pointers; see giql_hip_index).
struct IndexNearestView {
  IndexRowsView rows;     // first, key, bnd_key, n, n_chrom, wbits, uni_len (end_key / bnd_end are not read)
  const u32* chrom_lo;    // [n_chrom + 1] rank of first[c] among the keys
  const u32* rid;         // fixed-length form: the index's row ids (key order = (start, end) order)
  const u32* nr_pmax;     // general form: prefix max of the end keys in (start, end) order (NULL in the fixed form) ...
  const u32* nr_rid;      // ... and the row ids in that order
};

// #{v[j] < x}, inside the bucket the directory gives.
__device__ __forceinline__ u32 ir_rank1(const u32* __restrict__ v, const u32* __restrict__ bv, u32 x, u32 wbits) {
  const u32 cx = x >> wbits;
  return lower_bound_u32(v, bv[cx], bv[cx + 1], x);
}

// One thread per query row, in input order: idx_b_out[i] = the nearest indexed row (-1: none), dist_out[i] = its
// distance (0 with none).  *inverted is raised (never lowered) by a row with canonical end < start.
template <bool GENERAL>
__global__ __launch_bounds__(IR_NT) void k_index_nearest(const int* __restrict__ chrom, const int* __restrict__ start,
                                                          const int* __restrict__ end, u32 n, int start_off, int end_off,
                                                          IndexNearestView ix, int is_signed, i64 max_distance,
                                                          int32_t* __restrict__ idx_b_out, i64* __restrict__ dist_out,
                                                          u32* __restrict__ inverted) {
  __shared__ u32 s_first[MM_HIST_CHROMS + 1], s_clo[MM_HIST_CHROMS + 1];
  for (int k = threadIdx.x; k <= ix.rows.n_chrom && k <= MM_HIST_CHROMS; k += IR_NT) {
    s_first[k] = ix.rows.first[k];
    s_clo[k] = ix.chrom_lo[k];
  }
  __syncthreads();
  const u32 i = blockIdx.x * IR_NT + threadIdx.x;
  bool inv = false;
  if (i < n) {
    const int c = chrom[i];
    const i64 cs = (i64)start[i] + start_off, ce = (i64)end[i] + end_off;
    inv = ce < cs;
    u32 j = U32_MAX;  // the matched row in (start, end) order
    i64 best_d = 0;
    if (!inv && c >= 0 && c < ix.rows.n_chrom && s_clo[c + 1] > s_clo[c]) {
      const u32 blo = s_clo[c], bhi = s_clo[c + 1];
      const i64 base = (i64)s_first[c], width = (i64)s_first[c + 1] - base;
      const u32* __restrict__ key = ix.rows.key;
      const u32* __restrict__ bnd = ix.rows.bnd_key;
      auto key_of = [&](i64 local) -> u32 {  // a local coordinate as a key of the axis, clamped to the chromosome
        return (u32)(base + (local < 0 ? 0 : (local > width ? width : local)));
      };
      auto in_chrom = [&](u32 r) -> u32 { return r < blo ? blo : (r > bhi ? bhi : r); };
      u32 hi, lo2;
      i64 up_d = 0, dn_d = 0;
      u32 up = U32_MAX, dn = U32_MAX;
      bool overlap;
      if (GENERAL) {
        hi = in_chrom(ir_rank1(key, bnd, key_of(ce), ix.rows.wbits));
        lo2 = hi;
        const u32* __restrict__ pmax = ix.nr_pmax;
        const u32 m = hi > blo ? pmax[hi - 1] : 0u;  // largest end among the rows starting below a.end
        overlap = hi > blo && (i64)m - base > cs;
        if (overlap) {
          // first row in (start, end) order whose end exceeds a.start (cs < the largest end: only the clamp at 0 acts)
          j = gallop_back_upper_u32(pmax, blo, hi, key_of(cs));
        } else if (hi > blo) {  // m = the nearest upstream end (<= a.start): the first row that reaches it
          up = gallop_back_lower_u32(pmax, blo, hi, m);
          up_d = cs - ((i64)m - base) + 1;
        }
      } else {
        const i64 L = ix.rows.uni_len;
        ir_rank2(key, bnd, key_of(ce), key, bnd, key_of(cs - L + 1), ix.rows.wbits, hi, lo2);
        hi = in_chrom(hi);
        lo2 = in_chrom(lo2);
        overlap = lo2 < hi;  // rows with a.start - L < start < a.end
        if (overlap) {
          j = lo2;
        } else if (hi > blo) {
          const u32 k1 = key[hi - 1];  // the largest start below a.end: its end is the nearest upstream end
          up = gallop_back_lower_u32(key, blo, hi, k1);
          up_d = cs - ((i64)k1 - base + L) + 1;
        }
      }
      if (!overlap) {
        if (hi < bhi) {
          dn = hi;
          dn_d = ((i64)key[hi] - base) - ce + 1;
        }
        if (up != U32_MAX && (dn == U32_MAX || up_d <= dn_d)) {
          j = up;
          best_d = is_signed ? -up_d : up_d;
        } else if (dn != U32_MAX) {
          j = dn;
          best_d = dn_d;
        }
      }
      if (j != U32_MAX) {
        const i64 ad = best_d < 0 ? -best_d : best_d;
        if (max_distance >= 0 && ad > max_distance) j = U32_MAX;
      }
    }
    const int32_t best = j != U32_MAX ? (int32_t)(GENERAL ? ix.nr_rid[j] : ix.rid[j]) : -1;
    idx_b_out[i] = best;
    dist_out[i] = best < 0 ? 0 : best_d;
  }
  if (__ballot(inv) != 0ull && lane_id() == 0) *inverted = 1u;
}

}  // namespace giql
