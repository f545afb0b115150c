// giql_amd/csrc/index_rows_kernels.hip.h -- the per-row operators (COUNT / SEMI / ANTI) against a table INDEX.
//
// An index (giql_hip_index, giql_hip.hip) keeps a table's start keys fully sorted on a fixed axis: chromosome c owns
// the keys [first[c], first[c + 1]), every indexed row starts AND ends inside.  On that axis the count identity of
// k_count_rows (aux_kernels.hip.h) holds for a query row placed by the rules of k_index_query_keys:
//
//     count(a) = #{b.start_key < a.end_key} - #{b.end_key <= a.start_key}
//
// (rows of earlier chromosomes are in both terms, rows of later ones in neither).  Both terms are ranks in a sorted
// array: the index's start keys, and its end keys -- the start keys + L in the fixed-length form, a second sorted
// array in the general one.  A rank is found through a DIRECTORY, bnd[v] = first row with key >= v << wbits: two
// neighbouring cells bracket the rows of x's bucket (a few hundred for a genome-scale table), and the binary search
// runs only inside it.  So the query side is neither sorted nor scattered back: one thread per query row in INPUT
// order, the result written at the row's own index.  The directory (256 KiB at 2^16-key buckets) is read by every
// thread and is expected to stay in cache; what locality the searches have comes from the query table's own order.
// (An expectation, not a counter reading: what is measured is the call's time beside the ordinary operators',
// DESIGN.md "Row operators against an index".)
#pragma once

#include "dev_common.hip.h"
#include "join_kernels.hip.h"

namespace giql {

constexpr int IR_NT = 256;

// The 4 x 256 digit histogram of a plain u32 array (the general index's end keys, for their keys-only sort): what
// k_linearize counts on the way for the keys it builds.  Replicas as there: block b adds to replica b % n_replicas.
__global__ __launch_bounds__(IR_NT) void k_hist_u32(const u32* __restrict__ v, u32 n, u32* __restrict__ hist_partial,
                                                     u32 n_replicas) {
  __shared__ u32 s_hist[4 * 256];
  for (int k = threadIdx.x; k < 4 * 256; k += IR_NT) s_hist[k] = 0;
  __syncthreads();
  const u32 stride = gridDim.x * IR_NT;
  for (u32 i = blockIdx.x * IR_NT + threadIdx.x; i < n; i += stride) {
    const u32 k = v[i];
#pragma unroll
    for (int p = 0; p < 4; p++) atomicAdd(&s_hist[p * 256 + ((k >> (8 * p)) & 0xFFu)], 1u);
  }
  __syncthreads();
  u32* g = hist_partial + (size_t)(blockIdx.x % n_replicas) * 1024;
  for (int k = threadIdx.x; k < 4 * 256; k += IR_NT) {
    const u32 c = s_hist[k];
    if (c) atomicAdd(&g[k], c);
  }
}

// What the row kernels read of an index (all device pointers; see giql_hip_index).
struct IndexRowsView {
  const u32* first;     // [n_chrom + 1] chromosome bases on the axis
  const u32* key;       // [n] sorted start keys
  const u32* bnd_key;   // [2^(32 - wbits) + 1] directory over `key`
  const u32* end_key;   // general form: [n] sorted end keys (NULL in the fixed-length form) ...
  const u32* bnd_end;   // ... and their directory
  u32 n;
  int n_chrom;
  u32 wbits;
  i64 uni_len;          // the fixed canonical length (0 in the general form)
};

// A query row on the index's axis, by the rules of k_index_query_keys: start clamped to 0, end clamped to the
// chromosome's range; dead (matches nothing) when the chromosome is not in the index, the end lies at or below 0 or
// the start at or beyond the range.  An irregular row (canonical end <= start) on an indexed chromosome cannot be
// answered by ranks: *irr is set and the row is reported dead.
__device__ __forceinline__ bool ir_place(int c, i64 cs, i64 ce, int n_chrom, const u32* s_first, u32& ks, u32& ke,
                                         bool& irr) {
  if (c < 0 || c >= n_chrom) return false;
  const i64 lo = (i64)s_first[c], hi = (i64)s_first[c + 1];
  if (ce <= cs) {
    irr = true;
    return false;
  }
  if (ce <= 0 || lo + cs >= hi) return false;
  ks = (u32)(lo + (cs < 0 ? 0 : cs));
  const i64 e = lo + ce;
  ke = (u32)(e > hi ? hi : e);
  return true;
}

// #{v[j] < x} and #{w[j] < y} at once, each inside the bucket its directory gives: the two searches are independent,
// so their loads are issued together (a search is a chain of dependent loads, ~8 of them for a few hundred rows).
__device__ __forceinline__ void ir_rank2(const u32* __restrict__ v, const u32* __restrict__ bv, u32 x,
                                         const u32* __restrict__ w, const u32* __restrict__ bw, u32 y, u32 wbits,
                                         u32& rank_x, u32& rank_y) {
  const u32 cx = x >> wbits, cy = y >> wbits;
  u32 lo0 = bv[cx], hi0 = bv[cx + 1];
  u32 lo1 = bw[cy], hi1 = bw[cy + 1];
  while (lo0 < hi0 || lo1 < hi1) {
    const u32 m0 = lo0 + ((hi0 - lo0) >> 1), m1 = lo1 + ((hi1 - lo1) >> 1);
    const bool go0 = lo0 < hi0, go1 = lo1 < hi1;
    const u32 k0 = go0 ? v[m0] : 0u;
    const u32 k1 = go1 ? w[m1] : 0u;
    if (go0) {
      if (k0 < x) lo0 = m0 + 1; else hi0 = m0;
    }
    if (go1) {
      if (k1 < y) lo1 = m1 + 1; else hi1 = m1;
    }
  }
  rank_x = lo0;
  rank_y = lo1;
}

// One thread per query row, in input order.  FLAGS = false: counts_out[i] = overlapping indexed rows (int64);
// FLAGS = true: flag_out[i] = 1 when the row qualifies (SEMI: count > 0; ANTI: count == 0), for the scan +
// compaction that follows.  *irregular is raised (never lowered) when a row cannot be answered here.
template <bool FLAGS>
__global__ __launch_bounds__(IR_NT) void k_index_rows(const int* __restrict__ chrom, const int* __restrict__ start,
                                                       const int* __restrict__ end, u32 n, int start_off, int end_off,
                                                       IndexRowsView ix, int anti, i64* __restrict__ counts_out,
                                                       u32* __restrict__ flag_out, u32* __restrict__ irregular) {
  __shared__ u32 s_first[MM_HIST_CHROMS + 1];
  for (int k = threadIdx.x; k <= ix.n_chrom && k <= MM_HIST_CHROMS; k += IR_NT) s_first[k] = ix.first[k];
  __syncthreads();
  const u32 i = blockIdx.x * IR_NT + threadIdx.x;
  bool irr = false;
  if (i < n) {
    u32 ks = 0, ke = 0;
    const bool live = ir_place(chrom[i], (i64)start[i] + start_off, (i64)end[i] + end_off, ix.n_chrom, s_first, ks, ke, irr);
    u32 below = 0, done = 0;  // b.start_key < a.end_key; b.end_key <= a.start_key
    if (live) {
      if (ix.end_key) {
        // #{end_key <= ks} = #{end_key < ks + 1}  (ks < first[c + 1] <= the axis' end: no wrap)
        ir_rank2(ix.key, ix.bnd_key, ke, ix.end_key, ix.bnd_end, ks + 1u, ix.wbits, below, done);
      } else {
        // fixed length L: the sorted end keys are the sorted start keys + L, so
        // #{key + L <= ks} = #{key < ks - L + 1}; nothing lies below key 0
        const i64 t = (i64)ks - ix.uni_len + 1;
        ir_rank2(ix.key, ix.bnd_key, ke, ix.key, ix.bnd_key, t > 0 ? (u32)t : 0u, ix.wbits, below, done);
      }
    }
    if (FLAGS)
      flag_out[i] = ((below > done) != (anti != 0)) ? 1u : 0u;
    else
      counts_out[i] = (i64)below - (i64)done;
  }
  if (__ballot(irr) != 0ull && lane_id() == 0) *irregular = 1u;
}

}  // namespace giql
