// pair_expr_agg_kernels.hip.h -- aggregates of per-pair EXPRESSIONS over a join's pairs, per left row
// (include/giql_hip_pair_expr_agg.h): SUM(LEAST(a.end, b.end) - GREATEST(a.start, b.start)) ... GROUP BY a.*, the
// "Overlap Statistics" recipe (docs/recipes/advanced.rst) and what `bedtools intersect -wo | groupby` computes.
//
// The stage around it is pair_agg_kernels.hip.h's (check + load, the two sorts, heads, scan, scatter) and the
// reduction is merge_agg_kernels.hip.h's; what this header adds is ONE kernel, k_pxagg_tiles: k_magg_tiles whose
// value source may be a postfix program (select_kernels.hip.h: sel_eval_prog, DuckDB's semantics) evaluated at the
// pair (sorted_a[i], sorted_b[i]) instead of a column gathered through sorted_b[i].  The value goes from the
// interpreter straight into the segmented scan: a per-pair value array never exists in HBM (the composition
// eval_exprs -> pair_aggregate writes and reads 9 B per pair and expression, and holds 9 B x n_pairs per expression).
//
// Geometry and carries are k_magg_tiles': one block per MAGG_TILE sorted positions, one position per thread, wave64;
// per aggregate magg_reduce (the shared function) with its one barrier.  Every source of a thread is evaluated
// BEFORE the first barrier: the interpreter is __noinline__ and keeps its value stack in scratch, so a call between
// two barriers would stretch the time the block's waves wait on each other by a program's length per aggregate.
// Lanes past n evaluate nothing and still reach every barrier.  No atomics, no LDS beyond what k_magg_tiles declares.
//
// Ids: k_pagg_load has replaced every id outside its table by 0 (and raised the status word) before the sorts, so
// sorted_a[i] < n_a and sorted_b[i] < n_b hold for every live i: no program reads past a column.
#pragma once
#include "merge_agg_kernels.hip.h"
#include "select_kernels.hip.h"

namespace giql {

// A value source c is the program prog[c] where prog[c].count > 0, else the column M.cols[c].  For an expression
// source M.cols[c] = {nullptr, nullptr, GIQL_T_I64 or GIQL_T_F64}: k_magg_fold reads the type alone.
struct PxaggProg {
  int first, count;
};
struct PxaggArgs {
  MaggArgs M;
  PxaggProg prog[MAGG_MAX];
};

__global__ __launch_bounds__(MAGG_TILE) void k_pxagg_tiles(const u32* __restrict__ sorted_a,
                                                           const u32* __restrict__ sorted_b,
                                                           const u32* __restrict__ excl, const u32* __restrict__ flags,
                                                           u32 n, const DevOperand* __restrict__ nodes, PxaggArgs A) {
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
  const u32 ra = live ? sorted_a[i] : 0u, rb = live ? sorted_b[i] : 0u;
  const bool began_here = g != magg_region(excl, flags, t0) || flags[t0] != 0;
  const bool closed = gnext != g;
  const bool wave_end = live && (lane == WAVE - 1 || closed);
  if (lane == WAVE - 1) s_g[w] = g;
  u64 xs[MAGG_MAX];
  bool oks[MAGG_MAX];
#pragma unroll
  for (int c = 0; c < MAGG_MAX; c++) {  // (unrolled: xs / oks stay in registers)
    xs[c] = 0;
    oks[c] = false;
    if (c >= A.M.n_cols || !live) continue;
    const MaggCol col = A.M.cols[c];
    if (A.prog[c].count > 0) {
      const SelValue v = sel_eval_prog(nodes, A.prog[c].first, A.prog[c].count, (int)ra, (int)rb);
      oks[c] = !v.null;
      // an F64 source rounds an integer value once, as k_eval_expr does
      xs[c] = col.type == 3 ? (u64)__double_as_longlong(v.is_float ? v.f : (double)v.i) : (u64)v.i;
    } else {
      const bool ok = !col.valid || col.valid[rb] != 0;
      oks[c] = ok;
      if (ok) {
        if (col.type == 0) xs[c] = (u64)(i64) reinterpret_cast<const int*>(col.data)[rb];
        else if (col.type == 1) xs[c] = (u64) reinterpret_cast<const i64*>(col.data)[rb];
        else if (col.type == 2) xs[c] = (u64)__double_as_longlong((double)reinterpret_cast<const float*>(col.data)[rb]);
        else if (col.type == 3) xs[c] = reinterpret_cast<const u64*>(col.data)[rb];
      }
    }
  }
  int k = 0;
#pragma unroll
  for (int c = 0; c < MAGG_MAX; c++) {
    if (c >= A.M.n_cols) break;  // (kernel argument: the same in every lane)
    const bool flt = magg_is_float(A.M.cols[c].type);
    for (int a = 0; a < A.M.n_aggs; a++) {
      const MaggAgg ag = A.M.aggs[a];
      if (ag.col != c) continue;  // (uniform)
      magg_reduce(ag, flt, oks[c], xs[c], g, lane, w, wave_end, began_here, closed, k & 1, s_g, s_v, s_c);
      k++;
    }
  }
}

}  // namespace giql
