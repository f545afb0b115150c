// merge_agg_kernels.hip.h -- aggregates beside MERGE: COUNT(col), SUM, MIN, MAX per merged region.
//
// The reference keeps any plain aggregate beside MERGE and evaluates it under the per-cluster GROUP BY
// (src/giql/expanders/merge.py:317-390).  After cluster_front a merged region is a contiguous run of the
// sorted order, so the aggregate is ONE segmented reduction over values gathered through the row ids:
//   region of sorted position i:  g = excl[i] + flags[i] - 1;   value:  data[rids[i]], NULL when !valid[rids[i]].
//
// Reduce-by-key with carries, no atomics of any kind -- a float SUM is the same bits on every run:
//   k_magg_tiles  one block per tile of MAGG_TILE sorted positions.  Inside a wave a segmented inclusive scan (log
//                 shuffle steps, as k_merge_segmax); a run that crosses waves takes the earlier waves' tails from LDS,
//                 nearest wave last.  A region that begins and ends inside the tile is stored.  A tile's run of the
//                 region that reaches in from the tile before goes to the tile's `first` carry slot, the run that
//                 begins here and stays open at the tile's end to its `last` slot.
//   k_magg_fold   one wave per tile boundary that a region crosses AND whose region begins in the tile in front of
//                 it: last[t] + first[t + 1] + first[t + 2] + ... while the tiles still open with that region, 64
//                 tiles per step, combined by a fixed ladder of shuffles.  Every region has exactly one writer.
// Integer columns accumulate as int64, float columns are widened to binary64 on load; both travel as 64-bit
// patterns through one code path.  NaN follows DuckDB's total order (NaN above every number): MAX of a region with
// a NaN is NaN, MIN skips NaNs unless nothing else is there (NaN is MIN's identity), SUM propagates.
#pragma once
#include "dev_common.hip.h"

namespace giql {

constexpr int MAGG_TILE = 256;  // sorted positions per block, one per thread
constexpr int MAGG_MAX = 8;     // aggregates (and so distinct columns) per call
enum { MAGG_COUNT = 0, MAGG_SUM = 1, MAGG_MIN = 2, MAGG_MAX_ = 3 };  // = GIQL_AGG_*

struct MaggCol {
  const void* data;
  const unsigned char* valid;  // nullptr: all valid
  int type;                    // GIQL_T_I32 / I64 / F32 / F64, or MAGG_T_NONE
};
constexpr int MAGG_T_NONE = -1;  // a column read for its validity alone (COUNT over a column with no numeric data)
struct MaggAgg {
  int func, col;  // MAGG_*, index into cols
  u64* out;       // per region: the int64 / binary64 pattern (COUNT: the count)
  i64* out_nn;    // per region: non-NULL inputs (may be nullptr)
  u64 *first_v, *last_v;  // per tile carries
  i64 *first_c, *last_c;
};
struct MaggArgs {
  int n_cols, n_aggs;
  MaggCol cols[MAGG_MAX];
  MaggAgg aggs[MAGG_MAX];
};

__device__ __forceinline__ bool magg_is_float(int type) { return type >= 2; }  // GIQL_T_F32, GIQL_T_F64

__device__ __forceinline__ u64 magg_identity(int func, bool flt) {
  if (func == MAGG_MIN) return flt ? (u64)0x7FF8000000000000ull /* NaN */ : (u64)0x7FFFFFFFFFFFFFFFull;
  if (func == MAGG_MAX_) return flt ? (u64)0xFFF0000000000000ull /* -inf */ : (u64)0x8000000000000000ull;
  return 0;  // SUM: +0.0 and 0 share the pattern; COUNT carries no value
}

// a = the earlier part of the run, b = the later one
__device__ __forceinline__ u64 magg_combine(int func, bool flt, u64 a, u64 b) {
  if (func == MAGG_COUNT) return 0;
  if (flt) {
    const double x = __longlong_as_double((i64)a), y = __longlong_as_double((i64)b);
    double r;
    if (func == MAGG_SUM) r = x + y;
    else if (func == MAGG_MIN) r = x != x ? y : (y != y ? x : (y < x ? y : x));
    else r = (x != x || y != y) ? __longlong_as_double(0x7FF8000000000000ll) : (y > x ? y : x);
    return (u64)__double_as_longlong(r);
  }
  const i64 x = (i64)a, y = (i64)b;
  if (func == MAGG_SUM) return (u64)x + (u64)y;
  if (func == MAGG_MIN) return (u64)(y < x ? y : x);
  return (u64)(y > x ? y : x);
}

__device__ __forceinline__ u32 magg_region(const u32* __restrict__ excl, const u32* __restrict__ flags, u32 i) {
  return excl[i] + flags[i] - 1u;  // (every partition's first row is a head)
}

// One aggregate of one value source over the tile: the part every tile kernel shares (k_magg_tiles here,
// k_pxagg_tiles of pair_expr_agg_kernels.hip.h).  `x` / `ok` are the thread's value pattern and "is not NULL", `g` its
// region; s_g holds every wave's last region (written before the first call), s_v / s_c the waves' tails, in buffer
// `buf` (the callers alternate two: a wave one aggregate ahead writes the other one).  Holds one __syncthreads():
// every thread of the block calls it, for the same aggregates in the same order.
__device__ __forceinline__ void magg_reduce(const MaggAgg& ag, bool flt, bool ok, u64 x, u32 g, int lane, int w,
                                            bool wave_end, bool began_here, bool closed, int buf, const u32* s_g,
                                            u64 (*s_v)[MAGG_TILE / WAVE], u32 (*s_c)[MAGG_TILE / WAVE]) {
  u64 v = ok ? x : magg_identity(ag.func, flt);
  u32 cnt = ok ? 1u : 0u;
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const u64 ov = __shfl_up((unsigned long long)v, d);
    const u32 oc = (u32)__shfl_up((int)cnt, d);
    const u32 og = (u32)__shfl_up((int)g, d);
    if (lane >= d && og == g) {
      v = magg_combine(ag.func, flt, ov, v);
      cnt += oc;
    }
  }
  if (lane == WAVE - 1) {
    s_v[buf][w] = v;
    s_c[buf][w] = cnt;
  }
  __syncthreads();
  if (!wave_end) return;
  // g never decreases along the tile: an earlier wave whose tail is g is g to its end, and the run is contiguous
  for (int pw = w - 1; pw >= 0 && s_g[pw] == g; pw--) {
    v = magg_combine(ag.func, flt, s_v[buf][pw], v);
    cnt += s_c[buf][pw];
  }
  if (began_here && closed) {
    ag.out[g] = ag.func == MAGG_COUNT ? (u64)cnt : (cnt ? v : 0);  // (no non-NULL input: NULL, value 0)
    if (ag.out_nn) ag.out_nn[g] = (i64)cnt;
  } else if (closed || threadIdx.x == MAGG_TILE - 1) {  // (an open run ends at the tile's last thread)
    u64* cv = began_here ? ag.last_v : ag.first_v;
    i64* cc = began_here ? ag.last_c : ag.first_c;
    cv[blockIdx.x] = v;
    cc[blockIdx.x] = (i64)cnt;
  }
}

__global__ __launch_bounds__(MAGG_TILE) void k_magg_tiles(const u32* __restrict__ rids, const u32* __restrict__ excl,
                                                          const u32* __restrict__ flags, u32 n, MaggArgs A) {
  constexpr int NW = MAGG_TILE / WAVE;
  __shared__ u32 s_g[NW];
  __shared__ u64 s_v[2][NW];
  __shared__ u32 s_c[2][NW];
  const u32 t0 = blockIdx.x * MAGG_TILE;  // (< n: the grid is cdiv(n, MAGG_TILE))
  const u32 i = t0 + threadIdx.x;
  const bool live = i < n;
  const int lane = (int)lane_id(), w = (int)(threadIdx.x / WAVE);
  const u32 g = live ? magg_region(excl, flags, i) : 0xFFFFFFFFu;
  const u32 gnext = (live && i + 1 < n) ? magg_region(excl, flags, i + 1) : 0xFFFFFFFFu;
  const u32 r = live ? rids[i] : 0u;
  // the tile's first region began in an earlier tile unless the tile opens with a head
  const bool began_here = g != magg_region(excl, flags, t0) || flags[t0] != 0;
  const bool closed = gnext != g;                      // the region's last row
  const bool wave_end = live && (lane == WAVE - 1 || closed);
  if (lane == WAVE - 1) s_g[w] = g;
  int k = 0;
  for (int c = 0; c < A.n_cols; c++) {
    const MaggCol col = A.cols[c];
    const bool flt = magg_is_float(col.type);
    bool ok = live && (!col.valid || col.valid[r] != 0);
    u64 x = 0;
    if (ok) {
      if (col.type == 0) x = (u64)(i64) reinterpret_cast<const int*>(col.data)[r];
      else if (col.type == 1) x = (u64) reinterpret_cast<const i64*>(col.data)[r];
      else if (col.type == 2) x = (u64)__double_as_longlong((double)reinterpret_cast<const float*>(col.data)[r]);
      else if (col.type == 3) x = reinterpret_cast<const u64*>(col.data)[r];
    }
    for (int a = 0; a < A.n_aggs; a++) {
      const MaggAgg ag = A.aggs[a];
      if (ag.col != c) continue;  // (uniform)
      magg_reduce(ag, flt, ok, x, g, lane, w, wave_end, began_here, closed, k & 1, s_g, s_v, s_c);
      k++;
    }
  }
}

// one wave per tile t >= 0 with a boundary e = (t + 1) * MAGG_TILE < n
__global__ __launch_bounds__(256) void k_magg_fold(const u32* __restrict__ excl, const u32* __restrict__ flags, u32 n,
                                                   u32 n_tiles, MaggArgs A) {
  const u32 t = blockIdx.x * (256 / WAVE) + threadIdx.x / WAVE;
  const u64 e = ((u64)t + 1) * MAGG_TILE;
  if (e >= (u64)n || flags[e] != 0) return;  // (wave-uniform) no region crosses this boundary
  const u32 g = excl[e] - 1u;
  if (!(g != magg_region(excl, flags, t * MAGG_TILE) || flags[t * MAGG_TILE] != 0)) return;  // begins further left
  const int lane = (int)lane_id();
  for (int a = 0; a < A.n_aggs; a++) {
    const MaggAgg ag = A.aggs[a];
    const bool flt = magg_is_float(A.cols[ag.col].type);
    u64 acc = ag.last_v[t];
    i64 cnt = ag.last_c[t];
    for (u32 base = t + 1;; base += WAVE) {
      const u64 tt = (u64)base + lane;
      // tiles that still open inside region g: a prefix of the lanes
      const bool in = tt < n_tiles && flags[tt * MAGG_TILE] == 0 && excl[tt * MAGG_TILE] - 1u == g;
      u64 v = in ? ag.first_v[tt] : magg_identity(ag.func, flt);
      i64 c = in ? ag.first_c[tt] : 0;
#pragma unroll
      for (int d = 1; d < WAVE; d <<= 1) {  // lane L ends with lanes [0, L] combined in a fixed order
        const u64 ov = __shfl_up((unsigned long long)v, d);
        const i64 oc = __shfl_up((long long)c, d);
        if (lane >= d) {
          v = magg_combine(ag.func, flt, ov, v);
          c += oc;
        }
      }
      acc = magg_combine(ag.func, flt, acc, __shfl((unsigned long long)v, WAVE - 1));
      cnt += __shfl((long long)c, WAVE - 1);
      if (!__shfl((int)in, WAVE - 1)) break;  // the run ended within these 64 tiles
    }
    if (lane == 0) {
      ag.out[g] = ag.func == MAGG_COUNT ? (u64)cnt : (cnt ? acc : 0);
      if (ag.out_nn) ag.out_nn[g] = cnt;
    }
  }
}

}  // namespace giql
