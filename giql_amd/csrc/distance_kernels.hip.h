// giql_amd/csrc/distance_kernels.hip.h -- DISTANCE: the within-distance join's own stages and the per-pair value.
//
// The reference expands DISTANCE(a, b) into a CASE (src/giql/expanders/_distance.py:67-117; the AST twin is
// src/giql/expanders/distance.py:126-188, which of the four variants runs: distance.py:297-331):
//   NULL when the chromosomes differ [stranded: or a strand is NULL / '.' / '?'],
//   0    when a.start < b.end AND a.end > b.start,
//   b.start - a.end + 1   when a.end <= b.start   (B downstream of A),
//   a.start - b.end + 1   otherwise               (B upstream of A),
// with the sign rules of the variant applied AFTER the + 1.  The documented recipe "all pairs within N bp"
// (docs/dialect/distance-operators.rst:68-78, docs/recipes/distance.rst:60-73) filters a per-chromosome cartesian
// product by that CASE.
//
// For rows with start <= end on both sides and an integer N >= 0
//   DISTANCE(a, b) <= N   <=>   a.chrom = b.chrom AND a.start - N < b.end AND a.end + N > b.start,
// the literal overlap predicate with A widened by N on both ends (checked by brute force over every well-formed
// quadruple of 0..6 with N in 0..7; it does NOT hold for a row with end < start, which the plan refuses).  So the
// within-distance join is the INNER join's general two-class form over A' = [a.start - N, a.end + N):
//   * the span pass gives every chromosome ONE more position on either end of its range [cmin, cmax] (the minimum
//     and maximum over both sides' coordinates), whatever N is;
//   * k_window_linearize widens in 64-bit arithmetic and CLAMPS A' to [cmin - 1, cmax + 1].  Every B coordinate of
//     the chromosome lies in [cmin, cmax], so  max(a.start - N, cmin - 1) < b.end  <=>  a.start - N < b.end  and
//     likewise for the end: the clamp keeps the predicate for every B row of the chromosome, a widened row never
//     reaches a neighbouring chromosome's keys, and a large N does not inflate the 32-bit axis.  (A clamp at
//     coordinate 0 would be wrong: a = [3,5), b = [0,0), N = 10 has distance 4, and [0, 15) does not hold 0 strictly
//     inside.)
//   * a row that is zero-length AFTER widening (N = 0 and a.start = a.end) or a zero-length B row does not satisfy
//     the two-class identity; such rows take the sentinel key and the literal-predicate kernels below, as the
//     irregular rows of the INNER join do.
#pragma once

#include "dev_common.hip.h"
#include "join_kernels.hip.h"

namespace giql {

// keys[i] / ends[i] = the linearised, widened and clamped start / end of A row i; lo_pad / hi_pad = the span pass's
// padded offsets (the smallest canonical offset - 1, the largest + 1: chromosome c owns [gmin[c] + lo_pad,
// gmax[c] + hi_pad] on the axis, k_chrom_offsets was given the same two numbers).  Rows left zero-length get the
// sentinel key and a place in irr_list (meta->irr_a counts them).  hist_partial: the 64 replicas of the 4 x 256 digit
// histogram of the keys, as k_linearize leaves them for k_digit_offsets.  The host has read the span pass's status
// before this launch: every chrom id is in range (a bad one is skipped all the same) and no row has end < start.
__global__ __launch_bounds__(LIN_NT) void k_window_linearize(
    const int* __restrict__ chrom, const int* __restrict__ start, const int* __restrict__ end, u32 n, int start_off,
    int end_off, int n_chrom, const i64* __restrict__ chrom_base, const int* __restrict__ gmin,
    const int* __restrict__ gmax, int lo_pad, int hi_pad, i64 widen, u32* __restrict__ keys, u32* __restrict__ ends,
    u32* __restrict__ irr_list, DevMeta* __restrict__ meta, u32* __restrict__ hist_partial) {
  __shared__ u32 s_hist[4 * 256];
  for (int k = threadIdx.x; k < 4 * 256; k += LIN_NT) s_hist[k] = 0;
  __syncthreads();
  const u32 sentinel = meta->sentinel;
  const u32 stride = gridDim.x * LIN_NT;
  const u32 n_iter = (n + stride - 1) / stride;  // the same for every lane: the ballot below is full-wave
  const u32 i0 = blockIdx.x * LIN_NT + threadIdx.x;
  for (u32 it = 0; it < n_iter; it++) {
    const u64 i64_ = (u64)i0 + (u64)it * stride;
    const bool ok = i64_ < n;
    const u32 i = (u32)i64_;
    bool irr = false;
    u32 k = sentinel, ke = sentinel;
    if (ok) {
      const int c = chrom[i];
      if (c >= 0 && c < n_chrom) {
        const i64 lo = (i64)gmin[c] + lo_pad, hi = (i64)gmax[c] + hi_pad;
        i64 ws = (i64)start[i] + start_off - widen;
        i64 we = (i64)end[i] + end_off + widen;
        ws = ws < lo ? lo : ws;
        we = we > hi ? hi : we;
        irr = we <= ws;
        if (!irr) {
          const i64 b = chrom_base[c];
          k = (u32)(b + ws);
          ke = (u32)(b + we);
        }
      }
      keys[i] = k;
      ends[i] = ke;
#pragma unroll
      for (int p = 0; p < 4; p++) atomicAdd(&s_hist[p * 256 + ((k >> (8 * p)) & 0xFFu)], 1u);
    }
    const u64 m = __ballot(irr);
    if (m) {
      u32 base = 0;
      if (lane_id() == 0) base = atomicAdd(&meta->irr_a, (u32)__popcll(m));
      base = __shfl(base, 0, WAVE);
      if (irr) irr_list[base + (u32)__popcll(m & lanemask_lt())] = i;
    }
  }
  __syncthreads();
  u32* g = hist_partial + (size_t)(blockIdx.x % LIN_HIST_REPLICAS) * 1024;
  for (int k = threadIdx.x; k < 4 * 256; k += LIN_NT) {
    const u32 v = s_hist[k];
    if (v) atomicAdd(&g[k], v);
  }
}

// The widened literal predicate, all in 64 bits (widen <= 2^33, coordinates within the int32 range +- 1).
__device__ __forceinline__ bool literal_within(int ac, i64 as, i64 ae, int bc, i64 bs, i64 be, i64 widen) {
  return ac == bc && as - widen < be && ae + widen > bs;
}

// k_irr_count / k_irr_fill of the INNER join over the widened predicate.  Pairs involving an irregular row, each
// counted once (A is irregular when it is zero-length after widening: widen = 0 and start = end):
//   part X: (irregular a) x (every b)          -- thread per B row
//   part Y: (regular a)   x (irregular b)      -- thread per A row
// cnt has n_b + n_a entries [X | Y].
__global__ void k_window_irr_count(SideView a, SideView b, const u32* __restrict__ irr_a_list,
                                   const u32* __restrict__ irr_b_list, const DevMeta* __restrict__ meta, i64 widen,
                                   u32* __restrict__ cnt) {
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.n + b.n) return;
  u32 c = 0;
  if (t < b.n) {
    const int bc = b.chrom[t];
    const i64 bs = (i64)b.start[t] + b.start_off, be = (i64)b.end[t] + b.end_off;
    const u32 m = meta->irr_a;
    for (u32 k = 0; k < m; k++) {
      const u32 r = irr_a_list[k];
      c += literal_within(a.chrom[r], (i64)a.start[r] + a.start_off, (i64)a.end[r] + a.end_off, bc, bs, be, widen);
    }
  } else {
    const u32 i = t - b.n;
    const int ac = a.chrom[i];
    const i64 as = (i64)a.start[i] + a.start_off, ae = (i64)a.end[i] + a.end_off;
    if (ae + widen > as - widen) {
      const u32 m = meta->irr_b;
      for (u32 k = 0; k < m; k++) {
        const u32 r = irr_b_list[k];
        c += literal_within(ac, as, ae, b.chrom[r], (i64)b.start[r] + b.start_off, (i64)b.end[r] + b.end_off, widen);
      }
    }
  }
  cnt[t] = c;
}

__global__ void k_window_irr_fill(SideView a, SideView b, const u32* __restrict__ irr_a_list,
                                  const u32* __restrict__ irr_b_list, const DevMeta* __restrict__ meta, i64 widen,
                                  const u64* __restrict__ off, int32_t* __restrict__ row_a,
                                  int32_t* __restrict__ row_b) {
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.n + b.n) return;
  u64 o = off[t];
  if (t < b.n) {
    const int bc = b.chrom[t];
    const i64 bs = (i64)b.start[t] + b.start_off, be = (i64)b.end[t] + b.end_off;
    const u32 m = meta->irr_a;
    for (u32 k = 0; k < m; k++) {
      const u32 r = irr_a_list[k];
      if (literal_within(a.chrom[r], (i64)a.start[r] + a.start_off, (i64)a.end[r] + a.end_off, bc, bs, be, widen)) {
        row_a[o] = (int32_t)r;
        row_b[o] = (int32_t)t;
        o++;
      }
    }
  } else {
    const u32 i = t - b.n;
    const int ac = a.chrom[i];
    const i64 as = (i64)a.start[i] + a.start_off, ae = (i64)a.end[i] + a.end_off;
    if (ae + widen > as - widen) {
      const u32 m = meta->irr_b;
      for (u32 k = 0; k < m; k++) {
        const u32 r = irr_b_list[k];
        if (literal_within(ac, as, ae, b.chrom[r], (i64)b.start[r] + b.start_off, (i64)b.end[r] + b.end_off, widen)) {
          row_a[o] = (int32_t)i;
          row_b[o] = (int32_t)r;
          o++;
        }
      }
    }
  }
}

// ------------------------------------------------ the per-pair value
// dist_out[i] / valid_out[i] = DISTANCE(a[row_a[i]], b[row_b[i]]) for i < n: the CASE of _distance.py:67-117 on
// canonical coordinates, in 64 bits (coordinates at both ends of the int32 range are 2^32 apart).  valid_out[i] = 0
// is SQL NULL (dist_out[i] = 0 then).  flags bit 0 = signed, bit 1 = stranded; strand_a / strand_b hold one code per
// ROW of their table: 0 '+', 1 '-', anything else ('.', '?', NULL) makes the stranded value NULL.
// A row id outside its table raises GIQL_ERR_INVALID before any column is read (valid_out[i] = 0).
// HBM traffic per pair: 8 B of ids + 4 gathered coordinates and 2 chrom ids + 9 B written; the gathers dominate
// (a 64 B sector per 4 B value unless the pairs are grouped by row, which a join's output mostly is).
constexpr int DIST_NT = 256;
constexpr u32 DIST_FLAG_SIGNED = 1u, DIST_FLAG_STRANDED = 2u;

__global__ __launch_bounds__(DIST_NT) void k_pair_distance(SideView a, SideView b, const int* __restrict__ row_a,
                                                          const int* __restrict__ row_b, u64 n,
                                                          const int* __restrict__ strand_a,
                                                          const int* __restrict__ strand_b, u32 flags,
                                                          i64* __restrict__ dist_out, uint8_t* __restrict__ valid_out,
                                                          DevMeta* __restrict__ meta) {
  const u64 stride = (u64)gridDim.x * DIST_NT;
  const bool is_signed = flags & DIST_FLAG_SIGNED, stranded = flags & DIST_FLAG_STRANDED;
  bool bad = false;
  for (u64 i = (u64)blockIdx.x * DIST_NT + threadIdx.x; i < n; i += stride) {
    const int ia = ld_stream(row_a + i), ib = ld_stream(row_b + i);
    i64 d = 0;
    bool valid = false;
    if (ia < 0 || (u32)ia >= a.n || ib < 0 || (u32)ib >= b.n) {
      bad = true;
    } else {
      const int ac = a.chrom[ia], bc = b.chrom[ib];
      const i64 as = (i64)a.start[ia] + a.start_off, ae = (i64)a.end[ia] + a.end_off;
      const i64 bs = (i64)b.start[ib] + b.start_off, be = (i64)b.end[ib] + b.end_off;
      bool minus = false;
      valid = ac == bc;
      if (stranded) {
        const int sa = strand_a[ia], sb = strand_b[ib];
        valid = valid && (sa == 0 || sa == 1) && (sb == 0 || sb == 1);
        minus = sa == 1;
      }
      if (valid && !(as < be && ae > bs)) {
        if (ae <= bs) {                 // downstream: + by default, - on A's '-' strand
          d = bs - ae + 1;
          if (minus) d = -d;
        } else {                        // upstream
          d = as - be + 1;
          // unsigned: the strand flip only; signed: - by default, + on A's '-' strand
          if (is_signed ? !minus : minus) d = -d;
        }
      }
    }
    dist_out[i] = d;
    valid_out[i] = valid ? 1 : 0;
  }
  if (bad) atomicMin(&meta->status, -1);
}

}  // namespace giql
