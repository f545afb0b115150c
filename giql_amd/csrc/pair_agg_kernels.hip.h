// pair_agg_kernels.hip.h -- aggregates over a join's pairs, per left row: COUNT(col), SUM, MIN, MAX of B columns
// grouped by the A row of the pair (include/giql_hip_pair_agg.h; bedtools `map`).
//
// A post-pass over device pair arrays (row_a[i], row_b[i]).  The pairs are brought into (row_a, row_b) order by two
// stable radix sorts (radix_sort.hip.h: by row_b, then by row_a with row_b as the payload); after that the pairs of
// an A row are a contiguous run in ascending row_b, i.e. a "region" of merge_agg_kernels.hip.h, and the reduction IS
// k_magg_tiles / k_magg_fold with rids = the sorted row_b.  What this header adds is the stage around them:
//   k_pagg_load     checks every id against its table and lays the pairs out as the first sort's (key, end) columns.
//                   An id outside its table sets the status word and travels as 0: nothing downstream reads through it.
//   k_pagg_heads    flags[i] = the sorted row_a changes at i (the first position is a head).
//   k_pagg_scatter  one thread per sorted position; a head carries region g's results and its pair count to the
//                   outputs of row_a[head].  The outputs are zeroed before: a row without a pair reads 0 / NULL.
// All three are one-element-per-thread streaming kernels: no LDS, no atomics on values (the status word takes one
// atomicMin per block that met a bad id, as k_take), a handful of registers -- occupancy is not their limit, HBM is.
// Because the order inside a region is a function of the pair SET, a float SUM has the same bits whatever order the
// join produced the pairs in, and so has the zero a float MIN / MAX returns (it keeps the earlier of +0.0 and -0.0).
// The sort by row_b is skipped only where no aggregate reads a float value: integer sums, integer MIN / MAX and the
// counts do not depend on the order.
#pragma once
#include "dev_common.hip.h"

namespace giql {

constexpr int PAGG_NT = 256;

__global__ __launch_bounds__(PAGG_NT) void k_pagg_load(const int* __restrict__ row_a, const int* __restrict__ row_b,
                                                       u32 n, u32 n_a, u32 n_b, u32* __restrict__ key_b,
                                                       u32* __restrict__ pay_a, int* __restrict__ status) {
  const u32 i = blockIdx.x * PAGG_NT + threadIdx.x;
  bool bad = false;
  if (i < n) {
    u32 a = (u32)row_a[i], b = (u32)row_b[i];  // (a negative id is >= 2^31 > any table)
    if (a >= n_a) bad = true, a = 0;
    if (b >= n_b) bad = true, b = 0;
    key_b[i] = b;
    pay_a[i] = a;
  }
  if (__syncthreads_or(bad) && threadIdx.x == 0) atomicMin(status, -1 /* GIQL_ERR_INVALID */);
}

__global__ __launch_bounds__(PAGG_NT) void k_pagg_heads(const u32* __restrict__ sorted_a, u32 n,
                                                        u32* __restrict__ flags) {
  const u32 i = blockIdx.x * PAGG_NT + threadIdx.x;
  if (i < n) flags[i] = (i == 0 || sorted_a[i] != sorted_a[i - 1]) ? 1u : 0u;
}

struct PaggOut {
  const u64* seg_v;  // per region (k_magg_tiles / k_magg_fold wrote them)
  const i64* seg_c;
  u64* out;          // per A row
  i64* out_nn;       // may be nullptr
};
struct PaggScatter {
  int n_aggs;
  PaggOut a[8];
};

// head_pos[g]: the first sorted position of region g (k_merge_heads); *n_regions: the scan's total.
__global__ __launch_bounds__(PAGG_NT) void k_pagg_scatter(const u32* __restrict__ sorted_a,
                                                          const u32* __restrict__ flags,
                                                          const u32* __restrict__ excl,
                                                          const u32* __restrict__ head_pos,
                                                          const u64* __restrict__ n_regions, u32 n, u32 n_a,
                                                          i64* __restrict__ pairs_out, PaggScatter S) {
  const u32 i = blockIdx.x * PAGG_NT + threadIdx.x;
  if (i >= n || !flags[i]) return;
  const u32 g = excl[i];
  const u32 a = sorted_a[i];
  if (a >= n_a) return;  // (k_pagg_load left none)
  const u32 next = (u64)g + 1 < *n_regions ? head_pos[g + 1] : n;
  pairs_out[a] = (i64)(next - i);
  for (int k = 0; k < S.n_aggs; k++) {
    S.a[k].out[a] = S.a[k].seg_v[g];
    if (S.a[k].out_nn) S.a[k].out_nn[a] = S.a[k].seg_c[g];
  }
}

}  // namespace giql
