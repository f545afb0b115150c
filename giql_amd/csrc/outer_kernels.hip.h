// outer_kernels.hip.h -- the unmatched-row pass of a LEFT OUTER join (giql_hip_left_pad_dev).
//
// A LEFT join is the INNER join's pairs plus one (row_a, NULL) row per left row that keeps no pair.  The pairs
// are on the device already; these kernels find the left rows that do not occur among them and append
// (row, -1) entries behind the pairs, in place and in ascending row order:
//
//   k_left_mark   one flag byte per left row, set for every id met in row_a;
//   k_left_count  packs the flags into a bitmap of UNMATCHED rows (one bit per row) and counts them per block of
//                 LP_BLOCK_ROWS rows (k_scan_spine turns the block sums into offsets);
//   k_left_fill   every block expands the set bits of its words to row ids at n_pairs + its offset.
//
// The mark writes bytes with plain stores, not bits with atomicOr.  Measured (DESIGN.md "LEFT OUTER joins"): with
// the bits of a 100M-row table set by atomicOr after a plain test of the word, the whole pad -- mark, count and
// fill together; no kernel was timed on its own -- cost 9.6 ms behind 404M pairs and lost to the composition of
// older primitives; with flag bytes it costs 7.8 ms and wins.  The likely reason, not confirmed by any counter run:
// atomics on gfx950 execute at the memory side, one uncached request each, while a byte per row needs no
// read-modify-write.  Where the 100 MB of flags of such a table live between the mark and the count (L2, the
// Infinity Cache or HBM) was not measured either.  The count pass reads the bytes once, coalesced, and leaves the
// 12.5 MB bitmap the fill works from.  An id equal to its predecessor in row_a is skipped: the join writes a left
// row's pairs next to each other.
#pragma once
#include "dev_common.hip.h"

namespace giql {

constexpr int LP_NT = 256;
constexpr int LP_WORDS = 2;                              // 64-bit bitmap words per thread of a count / fill block
constexpr u32 LP_BLOCK_WORDS = (u32)LP_NT * LP_WORDS;    // words per block
constexpr u32 LP_BLOCK_ROWS = LP_BLOCK_WORDS * 64u;      // left rows per block (32768)

// flags[r] = 1 for every r = row_a[i].  Lane l of a wave reads element base + l (coalesced) and compares with
// lane l - 1's id: inside a run of one left row only the run's first lane of each wave stores.
__global__ __launch_bounds__(LP_NT) void k_left_mark(const int* __restrict__ row_a, u64 n, u32 n_rows,
                                                     uint8_t* __restrict__ flags, DevMeta* meta) {
  const u64 stride = (u64)gridDim.x * LP_NT;
  const u64 n_pad = (n + 63) & ~(u64)63;  // whole waves stay in the loop together (the shuffle below)
  bool bad = false;
  for (u64 i = (u64)blockIdx.x * LP_NT + threadIdx.x; i < n_pad; i += stride) {
    const int r = i < n ? ld_stream(row_a + i) : -1;
    const int prev = __shfl_up(r, 1, WAVE);
    if (i >= n) continue;
    if ((u32)r >= n_rows) {  // (negative ids included)
      bad = true;
      continue;
    }
    if (lane_id() != 0 && prev == r) continue;
    flags[r] = 1;
  }
  if (bad) atomicMin(&meta->status, -1 /* GIQL_ERR_INVALID */);
}

// zbits[w] bit l = row 64 w + l is inside the table and has no flag; bsums[block] = such rows among the block's
// LP_BLOCK_ROWS.  A wave takes LP_BLOCK_WORDS / 4 consecutive words, one coalesced 64-byte load and one ballot each.
__global__ __launch_bounds__(LP_NT) void k_left_count(const uint8_t* __restrict__ flags, u32 n_rows,
                                                      u64* __restrict__ zbits, u64* __restrict__ bsums) {
  constexpr u32 PER_WAVE = LP_BLOCK_WORDS / (LP_NT / WAVE);
  __shared__ u32 s_cnt[LP_NT / WAVE];
  const u64 n_words = ((u64)n_rows + 63) >> 6;
  const u64 w0 = (u64)blockIdx.x * LP_BLOCK_WORDS + (u64)wave_id() * PER_WAVE;
  u32 c = 0;  // (wave-uniform)
#pragma unroll 8
  for (u32 j = 0; j < PER_WAVE; j++) {
    const u64 w = w0 + j;
    if (w < n_words) {
      const u64 row = (w << 6) + lane_id();
      const u64 z = __ballot(row < n_rows && flags[row] == 0);
      if (lane_id() == 0) zbits[w] = z;
      c += (u32)__popcll(z);
    }
  }
  if (lane_id() == 0) s_cnt[wave_id()] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 t = 0;
    for (int w = 0; w < LP_NT / WAVE; w++) t += s_cnt[w];
    bsums[blockIdx.x] = t;
  }
}

__device__ __forceinline__ u32 lp_bcast(u32 v, int lane) {  // `lane` is wave-uniform
  return (u32)__builtin_amdgcn_readlane((int)v, lane);
}

// row_a[n_pairs + boff[block] + j] = the block's j-th unmatched row, row_b likewise = -1.  A block repeats its
// count as a prefix over its words (ascending: word k * LP_NT + t belongs to thread t in round k); a wave then
// expands its 64 words one at a time, lane l owning bit l, so the lanes of one store write adjacent entries.
// Output positions are 64-bit (n_pairs + offset may pass 2^31); the caller has checked them against the capacity.
__global__ __launch_bounds__(LP_NT) void k_left_fill(const u64* __restrict__ zbits, u32 n_rows,
                                                     const u64* __restrict__ boff, u64 n_pairs,
                                                     int* __restrict__ row_a, int* __restrict__ row_b) {
  __shared__ u32 lds[LP_NT / WAVE + 1];
  const u64 n_words = ((u64)n_rows + 63) >> 6;
  const u64 w0 = (u64)blockIdx.x * LP_BLOCK_WORDS;
  u64 pos = n_pairs + boff[blockIdx.x];
  for (int k = 0; k < LP_WORDS; k++) {
    const u64 w = w0 + (u64)k * LP_NT + threadIdx.x;
    const u64 z = w < n_words ? zbits[w] : 0;
    u32 total;
    const u32 pre = block_excl_scan<u32, LP_NT>((u32)__popcll(z), lds, total);
    if (total == 0) continue;  // (block-uniform)
    const u64 wave_w0 = w0 + (u64)k * LP_NT + (u64)wave_id() * WAVE;
    for (int s = 0; s < WAVE; s++) {
      const u64 zs = ((u64)lp_bcast((u32)(z >> 32), s) << 32) | lp_bcast((u32)z, s);
      if (zs == 0) continue;  // (wave-uniform)
      const u32 ps = lp_bcast(pre, s);
      if ((zs >> lane_id()) & 1ull) {
        const u64 o = pos + ps + (u32)__popcll(zs & lanemask_lt());
        row_a[o] = (int)(((wave_w0 + (u64)s) << 6) + lane_id());
        if (row_b) row_b[o] = -1;
      }
    }
    pos += total;
  }
}

}  // namespace giql
