// giql_amd/csrc/contain_kernels.hip.h -- column-to-column CONTAINS / WITHIN joins.
//
// The reference lowers `x.interval CONTAINS y.interval` to the naive predicate
//   x.chrom = y.chrom AND x.start <= y.start AND x.end >= y.end
// and WITHIN to the same with the operands exchanged (src/giql/expanders/intersects.py:155-166).  There is ONE device
// path, contain(outer, inner): the pairs (outer row, inner row) with the inner row inside the outer one.
//
// Regular rows (start < end) of both sides, on the join's linear axis: d inside c means
//   c.key <= d.key < d.endkey <= c.endkey,
// so every match of c lies in the contiguous run of the start-sorted inner side with d.key in [c.key, c.endkey): the
// "class 1" range of k_range_count (lo_off = 0), called the row's CANDIDATES here.  What is left is the filter
// d.endkey <= c.endkey:
//   * general form (k_ct_count / k_ct_fill): candidate-major.  The candidates of all outer rows, in sorted order, are
//     one sequence of T = sum(cand) positions cut into tiles of CT_TILE; a block owns a tile whatever rows it spans,
//     so a chromosome-long outer row with millions of candidates is spread over as many blocks as it needs and no
//     thread ever walks a row's range.  Count pass: one total per tile; u64 scan; fill pass: the same walk, a lane's
//     slot = tile offset + its ballot rank in the tile (stable inside a tile).
//   * uniform inner side (every inner row regular and L long): d.endkey <= c.endkey  <=>  d.key <= c.endkey - L, the
//     range [c.key, c.endkey - L + 1) is exact (k_contain_range_count) and the INNER join's scan + k_partition +
//     k_fill tail runs unchanged.
// Irregular rows (canonical end <= start) carry the sentinel key and lie outside both sorted prefixes; their pairs
// follow the literal predicate (k_contain_irr_count / k_contain_irr_fill), appended after the regular pairs.
#pragma once

#include "dev_common.hip.h"
#include "join_kernels.hip.h"

namespace giql {

// ------------------------------------------------ uniform inner side: the exact range
// k_range_count with a shifted UPPER bound: counts the S keys in [qs, qe + hi_off), hi_off = 1 - L.  An outer row
// shorter than L has qe + hi_off <= qs: SWindow::bounds searches `hi` from `lo`, so its count is 0, never negative
// (shift_key clamps at 0 as well).
template <int ITEMS, int CAP>
__global__ __launch_bounds__(RC_NT) void k_contain_range_count(
    const u32* __restrict__ qs, const u32* __restrict__ qe, u32 nq_total, const u32* __restrict__ irr_q,
    const u32* __restrict__ ss, u32 ns_total, const u32* __restrict__ irr_s, i64 hi_off,
    const u32* __restrict__ w_lo_arr, u32* __restrict__ lo_out, u32* __restrict__ cnt_out) {
  constexpr u32 TQ = RC_NT * ITEMS;
  __shared__ u32 s_tile[CAP];
  const u32 nq = nq_total - *irr_q;
  const u32 ns = ns_total - *irr_s;
  const u32 bid = blockIdx.x;
  const u32 q0 = bid * TQ;
  const u32 tid = threadIdx.x;
  u32 xs[ITEMS], xe[ITEMS];
#pragma unroll
  for (int i = 0; i < ITEMS; i++) {
    const u32 q = q0 + i * RC_NT + tid;
    const bool ok = q < nq;
    xs[i] = ok ? qs[q] : U32_MAX;
    xe[i] = ok ? shift_key(qe[q], hi_off) : U32_MAX;
  }
  const SWindow w = stage_window<CAP, RC_NT>(ss, ns, w_lo_arr[bid], w_lo_arr[bid + 1], s_tile);
#pragma unroll
  for (int i = 0; i < ITEMS; i++) {
    const u32 q = q0 + i * RC_NT + tid;
    if (q >= nq_total) continue;
    u32 lo = 0, hi = 0;
    if (q < nq) w.bounds(xs[i], xe[i], lo, hi);
    lo_out[q] = lo;
    cnt_out[q] = hi - lo;
  }
}

// ------------------------------------------------ general form: candidate tiles
// Tile shape after k_fill's (16384-pair tiles of 1024 threads beat 4096-pair tiles by 9 %; a tile
// starts with a chain of dependent loads -- partition, offsets, records -- that a larger tile amortises).  A wave
// owns CT_PER_WAVE consecutive candidates and walks them 64 at a time, so consecutive lanes read consecutive
// inner_end[j] inside a row (coalesced) and a window's passing lanes store to consecutive slots.
constexpr int CT_NT = 1024;
constexpr int CT_ITEMS = 16;
constexpr u32 CT_TILE = CT_NT * CT_ITEMS;                   // candidates per block
constexpr int CT_QCAP = 4096;                               // outer rows staged per tile (a quarter of its candidates)
constexpr u32 CT_PER_WAVE = CT_TILE / (CT_NT / WAVE);
constexpr int CT_NWIN = CT_PER_WAVE / WAVE;

// coff[nq + 1]: exclusive u64 offsets of the rows' candidate counts (coff[nq] = T); lo[q]: first candidate of sorted
// outer row q in the sorted inner side; part: k_partition(coff, tile = CT_TILE), the first outer row of each tile.
// The tile's rows {coff - tile base, lo, outer end key[, outer rid]} are staged in LDS (as k_fill stages its rows);
// candidate p of the tile belongs to the last staged row whose relative start is <= p, found by one binary search
// per lane for the wave's first window and by a step forward from there for the following ones.  A tile spanning
// more than CT_QCAP rows (long runs of rows without candidates) searches the offsets in HBM instead.
// FILL = false: tile_cnt[t] = candidates of tile t that pass inner_end[j] <= outer_end[q].
// FILL = true:  the passing candidates of tile t go to slots tile_off[t] + rank, rank = the candidate's position
//               among the tile's passing ones (wave totals through LDS, ballot rank inside a window).  Direct
//               stores: the passing lanes of a window write one contiguous run of each output array; staging a
//               tile's pairs in LDS for full-line stores would add 128 KB of LDS to a block that holds 64 KB of
//               row records, i.e. one block per CU instead of two.
template <bool FILL>
__device__ __forceinline__ void ct_tile_body(
    const u64* __restrict__ coff, const u32* __restrict__ lo, const u32* __restrict__ o_end,
    const u32* __restrict__ o_rid, u32 nq, const u32* __restrict__ i_end, const u32* __restrict__ i_rid,
    const u32* __restrict__ part, u64 n_cand, u32* __restrict__ tile_cnt, const u64* __restrict__ tile_off,
    int32_t* __restrict__ row_outer, int32_t* __restrict__ row_inner) {
  __shared__ u32 s_rel[CT_QCAP];    // relative candidate start of the row, clamped to [0, tile_len]
  __shared__ u32 s_jbase[CT_QCAP];  // lo - (coff - tile base) mod 2^32: inner index of candidate p = s_jbase + p
  __shared__ u32 s_oend[CT_QCAP];
  __shared__ u32 s_orid[FILL ? CT_QCAP : 1];
  __shared__ u32 s_wcnt[CT_NT / WAVE];
  const u32 tid = threadIdx.x, lane = lane_id(), wv = wave_id();
  const u32 bid = blockIdx.x;
  const u64 tile_start = (u64)bid * CT_TILE;
  const u64 rem = n_cand - tile_start;
  const u32 tile_len = rem < (u64)CT_TILE ? (u32)rem : CT_TILE;
  const u32 qf = part[bid];
  u32 ql = part[bid + 1];
  if (ql >= nq) ql = nq - 1;
  const u32 nqt = ql - qf + 1;
  const bool staged = nqt <= (u32)CT_QCAP;  // block-uniform
  if (staged) {
    for (u32 k = tid; k < nqt; k += CT_NT) {
      const u64 o = coff[qf + k];
      u32 r = 0;  // (row 0 starts at or before the tile: part[] is the LAST row with coff <= the tile base)
      if (o > tile_start) {
        const u64 d = o - tile_start;
        r = d > (u64)tile_len ? tile_len : (u32)d;
      }
      s_rel[k] = r;
      s_jbase[k] = lo[qf + k] - (u32)(o - tile_start);
      s_oend[k] = o_end[qf + k];
      if (FILL) s_orid[k] = o_rid[qf + k];
    }
  }
  __syncthreads();
  const u32 p_w0 = wv * CT_PER_WAVE;
  u32 jv[CT_NWIN], ev[CT_NWIN], xv[CT_NWIN], rv[FILL ? CT_NWIN : 1];
  // rows 1.. start inside the tile (rel >= 1); rows without candidates share their successor's start, and the LAST
  // row with rel <= p is the one that owns p
  u32 k = 0;
  if (staged && p_w0 < tile_len) k = upper_bound_u32(s_rel, 1, nqt, p_w0 + lane) - 1;
#pragma unroll
  for (int it = 0; it < CT_NWIN; it++) {
    const u32 p_rel = p_w0 + it * WAVE + lane;
    const bool ok = p_rel < tile_len;
    u32 j = 0, oe = 0, orid = 0;
    if (staged) {
      if (it > 0 && k + 1 < nqt && s_rel[k + 1] <= p_rel) k = upper_bound_u32(s_rel, k + 2, nqt, p_rel) - 1;
      j = s_jbase[k] + p_rel;
      oe = s_oend[k];
      if (FILL) orid = s_orid[k];
    } else if (ok) {
      const u64 p = tile_start + p_rel;
      const u32 q = (u32)(upper_bound_u64(coff, qf, (u64)ql + 1, p) - 1);
      j = lo[q] + (u32)(p - coff[q]);
      oe = o_end[q];
      if (FILL) orid = o_rid[q];
    }
    jv[it] = j;
    ev[it] = oe;
    if (FILL) rv[it] = orid;
    // issued here, compared below: the loads of a wave's windows fly together (j < the inner side's regular prefix
    // for every candidate: lo + cand <= ns in the range count)
    xv[it] = ok ? i_end[j] : U32_MAX;
  }
  u64 mask[CT_NWIN];
  u32 wtotal = 0;
#pragma unroll
  for (int it = 0; it < CT_NWIN; it++) {
    const bool ok = p_w0 + it * WAVE + lane < tile_len;
    mask[it] = __ballot(ok && xv[it] <= ev[it]);
    wtotal += (u32)__popcll(mask[it]);
  }
  if (lane == 0) s_wcnt[wv] = wtotal;
  __syncthreads();
  if (!FILL) {
    if (tid == 0) {
      u32 c = 0;
#pragma unroll
      for (int w = 0; w < CT_NT / WAVE; w++) c += s_wcnt[w];
      tile_cnt[bid] = c;
    }
    return;
  }
  u64 out = tile_off[bid];
  for (u32 w = 0; w < wv; w++) out += s_wcnt[w];
  const u64 below = lanemask_lt();
#pragma unroll
  for (int it = 0; it < CT_NWIN; it++) {
    const bool pass = (mask[it] >> lane) & 1ull;
    xv[it] = pass ? i_rid[jv[it]] : 0u;  // the gathers of all windows first, the stores after them
  }
#pragma unroll
  for (int it = 0; it < CT_NWIN; it++) {
    if ((mask[it] >> lane) & 1ull) {
      const u64 pos = out + (u64)__popcll(mask[it] & below);
      row_outer[pos] = (int32_t)rv[it];
      row_inner[pos] = (int32_t)xv[it];
    }
    out += (u64)__popcll(mask[it]);
  }
}

__global__ __launch_bounds__(CT_NT) void k_ct_count(
    const u64* __restrict__ coff, const u32* __restrict__ lo, const u32* __restrict__ o_end, u32 nq,
    const u32* __restrict__ i_end, const u32* __restrict__ part, u64 n_cand, u32* __restrict__ tile_cnt) {
  ct_tile_body<false>(coff, lo, o_end, nullptr, nq, i_end, nullptr, part, n_cand, tile_cnt, nullptr, nullptr, nullptr);
}

__global__ __launch_bounds__(CT_NT) void k_ct_fill(
    const u64* __restrict__ coff, const u32* __restrict__ lo, const u32* __restrict__ o_end,
    const u32* __restrict__ o_rid, u32 nq, const u32* __restrict__ i_end, const u32* __restrict__ i_rid,
    const u32* __restrict__ part, u64 n_cand, const u64* __restrict__ tile_off, int32_t* __restrict__ row_outer,
    int32_t* __restrict__ row_inner) {
  ct_tile_body<true>(coff, lo, o_end, o_rid, nq, i_end, i_rid, part, n_cand, nullptr, tile_off, row_outer, row_inner);
}

// ------------------------------------------------ irregular rows (literal predicate)
__device__ __forceinline__ bool literal_contains(int oc, i64 os, i64 oe, int ic, i64 is, i64 ie) {
  return oc == ic && os <= is && oe >= ie;
}

// k_irr_count / k_irr_fill of the INNER join over the containment predicate.  Pairs involving an irregular row, each
// counted once:
//   part X: (irregular outer) x (every inner)        -- thread per inner row
//   part Y: (regular outer)   x (irregular inner)    -- thread per outer row
// cnt has n_inner + n_outer entries [X | Y].
__global__ void k_contain_irr_count(SideView o, SideView in, const u32* __restrict__ irr_o_list,
                                    const u32* __restrict__ irr_i_list, const DevMeta* __restrict__ meta,
                                    u32* __restrict__ cnt) {
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= o.n + in.n) return;
  u32 c = 0;
  if (t < in.n) {
    const int ic = in.chrom[t];
    const i64 is = (i64)in.start[t] + in.start_off, ie = (i64)in.end[t] + in.end_off;
    const u32 m = meta->irr_a;
    for (u32 k = 0; k < m; k++) {
      const u32 r = irr_o_list[k];
      c += literal_contains(o.chrom[r], (i64)o.start[r] + o.start_off, (i64)o.end[r] + o.end_off, ic, is, ie);
    }
  } else {
    const u32 i = t - in.n;
    const int oc = o.chrom[i];
    const i64 os = (i64)o.start[i] + o.start_off, oe = (i64)o.end[i] + o.end_off;
    if (oe > os) {
      const u32 m = meta->irr_b;
      for (u32 k = 0; k < m; k++) {
        const u32 r = irr_i_list[k];
        c += literal_contains(oc, os, oe, in.chrom[r], (i64)in.start[r] + in.start_off, (i64)in.end[r] + in.end_off);
      }
    }
  }
  cnt[t] = c;
}

__global__ void k_contain_irr_fill(SideView o, SideView in, const u32* __restrict__ irr_o_list,
                                   const u32* __restrict__ irr_i_list, const DevMeta* __restrict__ meta,
                                   const u64* __restrict__ off, int32_t* __restrict__ row_outer,
                                   int32_t* __restrict__ row_inner) {
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= o.n + in.n) return;
  u64 w = off[t];
  if (t < in.n) {
    const int ic = in.chrom[t];
    const i64 is = (i64)in.start[t] + in.start_off, ie = (i64)in.end[t] + in.end_off;
    const u32 m = meta->irr_a;
    for (u32 k = 0; k < m; k++) {
      const u32 r = irr_o_list[k];
      if (literal_contains(o.chrom[r], (i64)o.start[r] + o.start_off, (i64)o.end[r] + o.end_off, ic, is, ie)) {
        row_outer[w] = (int32_t)r;
        row_inner[w] = (int32_t)t;
        w++;
      }
    }
  } else {
    const u32 i = t - in.n;
    const int oc = o.chrom[i];
    const i64 os = (i64)o.start[i] + o.start_off, oe = (i64)o.end[i] + o.end_off;
    if (oe > os) {
      const u32 m = meta->irr_b;
      for (u32 k = 0; k < m; k++) {
        const u32 r = irr_i_list[k];
        if (literal_contains(oc, os, oe, in.chrom[r], (i64)in.start[r] + in.start_off,
                             (i64)in.end[r] + in.end_off)) {
          row_outer[w] = (int32_t)i;
          row_inner[w] = (int32_t)r;
          w++;
        }
      }
    }
  }
}

}  // namespace giql
