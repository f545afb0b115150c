// coverage_kernels.hip.h -- the coverage profile of one table: DISJOIN's segments with their depth.
//
// The reference documents it as a GROUP BY over DISJOIN (docs/recipes/clustering.rst, "Reconstruct disjoin() Coverage
// Segments"; docs/recipes/disjoin.rst, "Build a Disjoint Partition"):
//   SELECT disjoin_chrom, disjoin_start, disjoin_end, COUNT(*) AS depth FROM DISJOIN(t) GROUP BY 1, 2, 3
// Grouping the pieces of self-mode DISJOIN by (chrom, start, end) gives, per pair of consecutive breakpoints x < y of
// a chromosome, the segment [x, y) with COUNT(*) = the rows with start <= x < end, where that number is not 0.  The
// breakpoint table of disjoin_kernels.hip.h holds all of it: after the event sort and its two scans, the last event i
// of a run of equal keys knows its breakpoint's index u = last_excl[i] and the depth behind it,
//   depth[u] = 2 * starts(0..i) - (i + 1)        (starts minus ends among the events <= bp[u]; exact, at most n).
// A segment starts at every breakpoint of depth > 0 and ends at the next breakpoint.  The last breakpoint of a
// chromosome has depth 0 (each of its rows has ended) and the keys of two chromosomes never meet (see the axis layout
// in disjoin_kernels.hip.h), so no segment crosses a chromosome and bp[u + 1] exists wherever depth[u] > 0.
//
// Run form (GIQL_COV_RUNS): maximal runs of abutting segments of equal depth become one row -- MERGE(interval,
// predicate := depth = PREV(depth)) over the segments.  Consecutive breakpoints of depth > 0 abut by construction, so
// breakpoint u continues the run of u - 1 exactly when depth[u - 1] == depth[u] > 0.  The head of a run writes chrom,
// start and depth; its tail (the next breakpoint does not continue it) writes the end into the head's row, whose index
// is the number of heads up to u, minus one.  One writer per cell: plain stores, no atomics.
#pragma once
#include "dev_common.hip.h"
#include "disjoin_kernels.hip.h"

namespace giql {

// bp[u], depth[u] at the last event of every run of equal keys; keep (NULL in the run form, whose flag needs the
// neighbour's depth): keep[u] = depth[u] > 0.  keep is zeroed by the caller past the breakpoints.
__global__ __launch_bounds__(256) void k_cov_depth(const u32* __restrict__ keys, const u32* __restrict__ last,
                                                   const u32* __restrict__ last_excl, const u32* __restrict__ is_start,
                                                   const u32* __restrict__ start_excl, u32 n_ev, u32* __restrict__ bp,
                                                   u32* __restrict__ depth, u32* __restrict__ keep) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_ev || !last[i]) return;
  const u32 u = last_excl[i];
  const u32 d = 2u * (start_excl[i] + is_start[i]) - (i + 1);
  bp[u] = keys[i];
  depth[u] = d;
  if (keep) keep[u] = d > 0 ? 1u : 0u;
}

// run form: keep[u] = breakpoint u heads a run
__global__ __launch_bounds__(256) void k_cov_run_heads(const u32* __restrict__ depth, const u64* __restrict__ n_bp,
                                                       u32* __restrict__ keep) {
  const u32 u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= (u32)*n_bp) return;
  const u32 d = depth[u];
  keep[u] = (d > 0 && !(u > 0 && depth[u - 1] == d)) ? 1u : 0u;
}

// one thread per breakpoint; slot[u] = exclusive scan of keep.  Coordinates go back into the side's declared encoding
// (as dj_piece).  depth_out may be NULL.
__global__ __launch_bounds__(256) void k_cov_fill(const u32* __restrict__ bp, const u32* __restrict__ depth,
                                                  const u32* __restrict__ keep, const u32* __restrict__ slot,
                                                  const u64* __restrict__ n_bp, const u32* __restrict__ chrom_first,
                                                  const i64* __restrict__ chrom_base, int n_chrom, int start_off,
                                                  int end_off, int runs, u32 total, int* __restrict__ out_chrom,
                                                  int* __restrict__ out_start, int* __restrict__ out_end,
                                                  i64* __restrict__ out_depth) {
  const u32 u = blockIdx.x * blockDim.x + threadIdx.x;
  const u32 U = (u32)*n_bp;
  if (u >= U || u + 1 >= U) return;  // (the last breakpoint starts nothing)
  const u32 d = depth[u];
  if (d == 0) return;
  const u32 key = bp[u];
  const u32 c = upper_bound_u32(chrom_first, 0, (u32)n_chrom + 1, key) - 1;
  const u32 k = keep[u], g = slot[u];
  if (c >= (u32)n_chrom || g + k == 0 || g + k > total) return;  // (never, on rows the call has checked)
  const i64 b = chrom_base[c];
  if (k) {
    out_chrom[g] = (int)c;
    out_start[g] = (int)((i64)key - b - start_off);
    if (out_depth) out_depth[g] = (i64)d;
  }
  if (!runs || depth[u + 1] != d) out_end[g + k - 1] = (int)((i64)bp[u + 1] - b - end_off);
}

}  // namespace giql
