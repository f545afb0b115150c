// giql_amd/csrc/row_pred_kernels.hip.h -- SEMI / ANTI existence and per-row COUNT over the three pair predicates
// that are not INTERSECTS:
//   a CONTAINS b          a.chrom = b.chrom AND a.start <= b.start AND a.end >= b.end
//   a WITHIN b            the same with the operands exchanged
//   DISTANCE(a, b) <= N   the overlap predicate with A widened by N (distance_kernels.hip.h)
//
// EXISTENCE is one sort of B, one prefix maximum and one binary search per A row, as for INTERSECTS
// (aux_kernels.hip.h), with every row of both sides on its real key (no start < end assumption is used):
//   a WITHIN some b    <=>  max{ b.endkey : b.key <= a.key } >= a.endkey        B sorted by start, pmax over its ends
//   a CONTAINS some b  <=>  max{ b.key : b.endkey <= a.endkey } >= a.key        B sorted by END, pmax over its starts
//   DISTANCE <= N      <=>  k_semi_flags over the widened, clamped A keys (k_rp_window_keys)
// The linear axis does not leak between chromosomes: k_chrom_offsets gives a chromosome max - min + 1 positions over
// BOTH sides' starts and ends, so for any row, inverted ones included, base <= key and endkey <= base + max - min <
// the next base.  A row of a later chromosome has both keys above a.endkey and a row of an earlier one has both keys
// below a.key: neither can satisfy either test.  The prefix maximum is taken over a set that may hold earlier
// chromosomes' rows; their keys are smaller than any on a's chromosome, so they cannot turn a miss into a hit.
//
// COUNT over DISTANCE is k_count_rows' rank difference over the widened keys; COUNT over CONTAINS / WITHIN is a
// two-sided dominance count, for which no rank difference exists: the candidate-tile walk of contain_kernels.hip.h
// accumulating per ROW instead of per tile (k_ct_rows).  Irregular rows follow the literal predicate in every form.
#pragma once

#include "aux_kernels.hip.h"
#include "contain_kernels.hip.h"
#include "dev_common.hip.h"
#include "distance_kernels.hip.h"
#include "join_kernels.hip.h"

namespace giql {

constexpr int RP_CONTAINS = 1, RP_WITHIN = 2, RP_DISTANCE = 3;  // GIQL_ROWPRED_* of the C ABI

// P(x, y), the literal predicate on canonical coordinates (widen is read for RP_DISTANCE only).
__device__ __forceinline__ bool literal_rowpred(int pred, int xc, i64 xs, i64 xe, int yc, i64 ys, i64 ye, i64 widen) {
  if (pred == RP_CONTAINS) return literal_contains(xc, xs, xe, yc, ys, ye);
  if (pred == RP_WITHIN) return literal_contains(yc, ys, ye, xc, xs, xe);
  return literal_within(xc, xs, xe, yc, ys, ye, widen);
}

// ------------------------------------------------------------- SEMI / ANTI
// Queries are the A rows sorted (coarsely: locality only) by linearised start; flag[rid] = 1 when the row qualifies.
// within = 1: b_sorted = B's start keys ascending, b_pmax = running max of its end keys in that order;
//             j = #{b.key <= a.key}, hit = pmax[j - 1] >= a.endkey.
// within = 0 (CONTAINS): b_sorted = B's END keys ascending, b_pmax = running max of its start keys in that order;
//             j = #{b.endkey <= a.endkey}, hit = pmax[j - 1] >= a.key.
__global__ __launch_bounds__(256) void k_rp_semi_flags(const u32* __restrict__ a_keys, const u32* __restrict__ a_ends,
                                                        const u32* __restrict__ a_rids, u32 n_a,
                                                        const DevMeta* __restrict__ meta,
                                                        const u32* __restrict__ b_sorted,
                                                        const u32* __restrict__ b_pmax, u32 n_b, int within, int anti,
                                                        u32* __restrict__ flag) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_a) return;
  const u32 qs = a_keys[i], qe = a_ends[i];
  bool hit = false;
  if (n_b > 0 && qs < meta->sentinel) {  // rows with a bad chrom id carry the sentinel
    const u32 j = upper_bound_u32(b_sorted, 0, n_b, within ? qs : qe);
    hit = j > 0 && b_pmax[j - 1] >= (within ? qe : qs);
  }
  flag[a_rids[i]] = (hit != (anti != 0)) ? 1u : 0u;
}

// k_window_linearize for the existence test: the widened, clamped keys of EVERY A row.  A row that stays zero-length
// (N = 0 and start = end) keeps its real key instead of the sentinel: k_semi_flags is the literal overlap test, exact
// for such a row (a = [5,5), b = [3,8), N = 0: distance 0, and 3 < 5 with pmax 8 > 5).  Only a bad chrom id gets the
// sentinel.  For N > 0 the clamp never empties a row: its coordinates lie in [cmin, cmax] and the clamp range is
// [cmin - 1, cmax + 1].
__global__ __launch_bounds__(LIN_NT) void k_rp_window_keys(
    const int* __restrict__ chrom, const int* __restrict__ start, const int* __restrict__ end, u32 n, int start_off,
    int end_off, int n_chrom, const i64* __restrict__ chrom_base, const int* __restrict__ gmin,
    const int* __restrict__ gmax, int lo_pad, int hi_pad, i64 widen, u32* __restrict__ keys, u32* __restrict__ ends,
    const DevMeta* __restrict__ meta, u32* __restrict__ hist_partial) {
  __shared__ u32 s_hist[4 * 256];
  for (int k = threadIdx.x; k < 4 * 256; k += LIN_NT) s_hist[k] = 0;
  __syncthreads();
  const u32 sentinel = meta->sentinel;
  const u64 stride = (u64)gridDim.x * LIN_NT;
  for (u64 i = (u64)blockIdx.x * LIN_NT + threadIdx.x; i < n; i += stride) {
    u32 k = sentinel, ke = sentinel;
    const int c = chrom[i];
    if (c >= 0 && c < n_chrom) {
      const i64 lo = (i64)gmin[c] + lo_pad, hi = (i64)gmax[c] + hi_pad;
      i64 ws = (i64)start[i] + start_off - widen;
      i64 we = (i64)end[i] + end_off + widen;
      ws = ws < lo ? lo : ws;
      we = we > hi ? hi : we;
      const i64 b = chrom_base[c];
      k = (u32)(b + ws);
      ke = (u32)(b + we);
    }
    keys[i] = k;
    ends[i] = ke;
#pragma unroll
    for (int p = 0; p < 4; p++) atomicAdd(&s_hist[p * 256 + ((k >> (8 * p)) & 0xFFu)], 1u);
  }
  __syncthreads();
  u32* g = hist_partial + (size_t)(blockIdx.x % LIN_HIST_REPLICAS) * 1024;
  for (int k = threadIdx.x; k < 4 * 256; k += LIN_NT) {
    const u32 v = s_hist[k];
    if (v) atomicAdd(&g[k], v);
  }
}

// rows_out = 0 .. n - 1: the ANTI result of a predicate no pair satisfies (max_distance = -1).
__global__ __launch_bounds__(256) void k_rp_iota(int32_t* __restrict__ rows_out, u32 n) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) rows_out[i] = (int32_t)i;
}

// ------------------------------------------------------ COUNT over DISTANCE
// k_count_rows over the widened keys of k_window_linearize: #{b.key < a'.endkey} - #{b.endkey <= a'.key} over the
// regular B rows (two keys-only sorts of B), literal_within against the zero-length B rows.  The A rows that stay
// zero-length carry the sentinel and are settled by k_rp_count_irregular.
__global__ __launch_bounds__(256) void k_rp_count_window_rows(
    const u32* __restrict__ a_keys, const u32* __restrict__ a_ends, const u32* __restrict__ a_rids, u32 n_a_total,
    SideView a, SideView b, const u32* __restrict__ b_keys_sorted, const u32* __restrict__ b_ends_sorted,
    u32 n_b_total, const u32* __restrict__ irr_b_list, const DevMeta* __restrict__ meta, i64 widen,
    i64* __restrict__ counts_out) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_a_total) return;
  const u32 n_reg = n_b_total - meta->irr_b;
  const u32 qs = a_keys[i], qe = a_ends[i], r = a_rids[i];
  if (qs >= meta->sentinel) return;  // zero-length after widening (or a bad chrom id)
  const u32 below = lower_bound_u32(b_keys_sorted, 0, n_reg, qe);
  const u32 done = upper_bound_u32(b_ends_sorted, 0, n_reg, qs);
  i64 cnt = (i64)below - (i64)done;
  const u32 m = meta->irr_b;
  if (m) {  // rare: the literal predicate against the zero-length B rows
    const int ac = a.chrom[r];
    const i64 as = (i64)a.start[r] + a.start_off, ae = (i64)a.end[r] + a.end_off;
    for (u32 k = 0; k < m; k++) {
      const u32 rb = irr_b_list[k];
      cnt += literal_within(ac, as, ae, b.chrom[rb], (i64)b.start[rb] + b.start_off, (i64)b.end[rb] + b.end_off,
                            widen);
    }
  }
  counts_out[r] = cnt;
}

// ------------------------------------------------ irregular rows (literal predicate)
// One block per listed X row: counts_out[r] = #{y : P(x, y)} over EVERY Y row (k_count_irregular over any predicate).
// The regular path leaves nothing in a listed row's count, so the total is stored, not added.
__global__ __launch_bounds__(256) void k_rp_count_irregular(SideView x, SideView y, const u32* __restrict__ irr_x_list,
                                                             int pred, i64 widen, i64* __restrict__ counts_out) {
  __shared__ u64 lds[256 / WAVE];
  const u32 r = irr_x_list[blockIdx.x];
  const int xc = x.chrom[r];
  const i64 xs = (i64)x.start[r] + x.start_off, xe = (i64)x.end[r] + x.end_off;
  u64 c = 0;
  for (u32 j = threadIdx.x; j < y.n; j += 256)
    c += literal_rowpred(pred, xc, xs, xe, y.chrom[j], (i64)y.start[j] + y.start_off, (i64)y.end[j] + y.end_off,
                         widen);
  c = wave_reduce_sum(c);
  if (lane_id() == 0) lds[wave_id()] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 t = 0;
#pragma unroll
    for (int w = 0; w < 256 / WAVE; w++) t += lds[w];
    counts_out[r] = (i64)t;
  }
}

// Thread per REGULAR X row (canonical end > start): counts_out[x] += #{listed y : P(x, y)}.  Launched after the regular
// path on the same stream; one thread owns a row, so the add needs no atomic.
__global__ __launch_bounds__(256) void k_rp_count_vs_irregular(SideView x, SideView y,
                                                                const u32* __restrict__ irr_y_list,
                                                                const u32* __restrict__ n_irr_y, int pred,
                                                                i64* __restrict__ counts_out) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= x.n) return;
  const int xc = x.chrom[i];
  const i64 xs = (i64)x.start[i] + x.start_off, xe = (i64)x.end[i] + x.end_off;
  if (xe <= xs) return;
  const u32 m = *n_irr_y;
  i64 c = 0;
  for (u32 k = 0; k < m; k++) {
    const u32 r = irr_y_list[k];
    c += literal_rowpred(pred, xc, xs, xe, y.chrom[r], (i64)y.start[r] + y.start_off, (i64)y.end[r] + y.end_off, 0);
  }
  if (c) counts_out[i] += c;
}

// ------------------------------------------- COUNT over CONTAINS / WITHIN: candidate tiles
// ct_tile_body's walk (contain_kernels.hip.h: coff, lo, part, the staged row records, CT_* shapes) with the passing
// candidates accumulated per ROW.  Integer atomics: the result does not depend on the order the adds arrive in.
// PER_INNER = false (a CONTAINS b, a = outer): cnt64[o_rid[q]] += the passing candidates of sorted outer row q.
//   Inside a 64-candidate window the lanes of one row are contiguous: the head lane of each run reduces the run's
//   passing lanes from the ballot and adds ONCE per (window, row) to the row's LDS counter; after the tile, one
//   global atomicAdd per (tile, row with a non-zero sum) -- a row's candidates may span tiles, so the host zeroes
//   cnt64 first.  The row ids are read from HBM at the flush.  A tile spanning more than CT_QCAP rows makes the same
//   per-run reduction and adds to global memory directly.
//   Static LDS: 3 staged arrays + the counters = 4 x CT_QCAP x 4 B = 64 KB, k_ct_fill's four staged arrays without
//   its wave totals: two blocks per CU still fit.
// PER_INNER = true (a WITHIN b, a = inner): cnt32[j] += 1 for a passing candidate at position j of the SORTED inner
//   side (consecutive lanes of a row hit consecutive addresses); k_rp_scatter_counts then writes counts_out[i_rid[j]].
template <bool PER_INNER>
__global__ __launch_bounds__(CT_NT) void k_ct_rows(
    const u64* __restrict__ coff, const u32* __restrict__ lo, const u32* __restrict__ o_end,
    const u32* __restrict__ o_rid, u32 nq, const u32* __restrict__ i_end, const u32* __restrict__ part, u64 n_cand,
    unsigned long long* __restrict__ cnt64, u32* __restrict__ cnt32) {
  __shared__ u32 s_rel[CT_QCAP];    // relative candidate start of the row, clamped to [0, tile_len]
  __shared__ u32 s_jbase[CT_QCAP];  // lo - (coff - tile base) mod 2^32: inner index of candidate p = s_jbase + p
  __shared__ u32 s_oend[CT_QCAP];
  __shared__ u32 s_cnt[PER_INNER ? 1 : CT_QCAP];  // passing candidates of the staged row inside this tile
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
      if (!PER_INNER) s_cnt[k] = 0;
    }
  }
  __syncthreads();
  const u32 p_w0 = wv * CT_PER_WAVE;
  u32 jv[CT_NWIN], ev[CT_NWIN], xv[CT_NWIN], kv[PER_INNER ? 1 : CT_NWIN];
  u32 k = 0;
  if (staged && p_w0 < tile_len) k = upper_bound_u32(s_rel, 1, nqt, p_w0 + lane) - 1;
#pragma unroll
  for (int it = 0; it < CT_NWIN; it++) {
    const u32 p_rel = p_w0 + it * WAVE + lane;
    const bool ok = p_rel < tile_len;
    u32 j = 0, oe = 0, row = U32_MAX;  // row: the staged index (staged) or the sorted outer row (un-staged) of the lane
    if (staged) {
      if (it > 0 && k + 1 < nqt && s_rel[k + 1] <= p_rel) k = upper_bound_u32(s_rel, k + 2, nqt, p_rel) - 1;
      j = s_jbase[k] + p_rel;
      oe = s_oend[k];
      row = k;
    } else if (ok) {
      const u64 p = tile_start + p_rel;
      const u32 q = (u32)(upper_bound_u64(coff, qf, (u64)ql + 1, p) - 1);
      j = lo[q] + (u32)(p - coff[q]);
      oe = o_end[q];
      row = q;
    }
    jv[it] = j;
    ev[it] = oe;
    if (!PER_INNER) kv[it] = row;
    // issued here, compared below: the loads of a wave's windows fly together (j < the inner side's regular prefix
    // for every candidate: lo + cand <= ns in the range count)
    xv[it] = ok ? i_end[j] : U32_MAX;
  }
#pragma unroll
  for (int it = 0; it < CT_NWIN; it++) {
    const bool ok = p_w0 + it * WAVE + lane < tile_len;
    const bool pass = ok && xv[it] <= ev[it];
    if (PER_INNER) {
      if (pass) atomicAdd(&cnt32[jv[it]], 1u);
    } else {
      const u64 mask = __ballot(pass);
      if (mask == 0ull) continue;  // wave-uniform
      const u32 row = kv[it];
      const u32 prev = __shfl_up(row, 1, WAVE);
      const u64 heads = __ballot(lane == 0 || prev != row);
      if ((heads >> lane) & 1ull) {
        // the run [lane, next head): its passing lanes
        const u64 above = lane == WAVE - 1 ? 0ull : heads & ~((2ull << lane) - 1ull);
        const u64 upto = above ? ((1ull << __builtin_ctzll(above)) - 1ull) : ~0ull;
        const u32 c = (u32)__popcll(mask & upto & ~lanemask_lt());
        if (c) {
          if (staged)
            atomicAdd(&s_cnt[row], c);
          else
            atomicAdd(&cnt64[o_rid[row]], (unsigned long long)c);
        }
      }
    }
  }
  if (PER_INNER || !staged) return;  // block-uniform
  __syncthreads();
  for (u32 q = tid; q < nqt; q += CT_NT) {
    const u32 c = s_cnt[q];
    if (c) atomicAdd(&cnt64[o_rid[qf + q]], (unsigned long long)c);
  }
}

// counts_out[rid[j]] = cnt32[j] over the sorted side (per-inner counts; the uniform form's exact range counts).
__global__ __launch_bounds__(256) void k_rp_scatter_counts(const u32* __restrict__ cnt32, const u32* __restrict__ rid,
                                                            u32 n, i64* __restrict__ counts_out) {
  const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) counts_out[rid[j]] = (i64)cnt32[j];
}

}  // namespace giql
