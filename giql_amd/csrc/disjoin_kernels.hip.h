// disjoin_kernels.hip.h -- DISJOIN: every target row cut at the reference's breakpoints.
//
// The reference lowers DISJOIN(target [, reference := ref]) to five CTEs with two UNIONs, a LEAD
// window and a correlated EXISTS (src/giql/expanders/disjoin.py:147-202):
//   breakpoints = DISTINCT (chrom, pos) over every reference start and every reference end
//   cuts        = target JOIN breakpoints ON chrom AND start < pos AND pos < end       (strict)
//   pieces      = consecutive gaps of {start} UNION cuts UNION {end} per target row     (LEAD)
//   kept        = pieces [x, y) with EXISTS (reference row: r.start <= x AND r.end > x)  (skipped in self mode)
// Here, on the linearised axis of the join (k_chrom_offsets):
//   events : the 2 * n_ref keys {start} ++ {end} of the reference, sorted once with the key sort; the row id
//            the sort carries says which half an event came from (id < n_ref: a start);
//   bp[u]  : the distinct keys (last event of every run of equal keys, compacted through a scan);
//   cov[u] : (starts <= bp[u]) - (ends <= bp[u]) > 0 -- the number of reference rows with
//            start <= bp[u] < end, from ONE scan of the start bit over the sorted events: at sorted index i
//            it is 2 * starts(0..i) - (i + 1).  Exact because every reference row has start <= end (checked
//            here, on the device).  The depth is constant between breakpoints, so a piece starting at x is
//            covered iff cov[upper_bound(bp, x) - 1]; zero-length reference rows cut and never cover;
//   count  : per target row, in INPUT order: lo = upper_bound(bp, s), hi = lower_bound(bp, e),
//            first = covered(s), count = first + ncov[hi] - ncov[lo]   (self mode: hi - lo + 1);
//   fill   : OUTPUT-major -- a block takes 1,024 consecutive output slots, finds their parent rows by binary
//            search in the (LDS-staged) output offsets and resolves each piece in O(1) from bp / the list
//            of covered breakpoints: a chromosome-long target over millions of breakpoints is spread over
//            as many blocks as it has pieces.
//
// Axis layout: k_chrom_offsets gives chromosome c the keys [first[c], first[c + 1]) with
// first[c + 1] - first[c] = (max end + off_max) - (min start + off_min) + 1 over BOTH sides, and every
// canonical start and end of a row with start <= end lies in [min start + off_min, max end + off_max]: the
// keys of two chromosomes never meet, not even at a boundary (the + 1 keeps the largest end of c below
// first[c + 1]).  A target row's keys ks <= ke are both in its chromosome's range, so a breakpoint p with
// ks < p < ke is a breakpoint of the same chromosome; and the depth left behind by an earlier chromosome
// is 0 (each of its rows has ended), so the "first piece" test never sees another chromosome's coverage.
#pragma once
#include "dev_common.hip.h"
#include "join_kernels.hip.h"

namespace giql {

constexpr u32 DJ_BAD_TARGET = 1u, DJ_BAD_REFERENCE = 2u;  // DevMeta::aux0: a row with canonical end < start
constexpr u32 DJ_FIRST = 0x80000000u;                     // lo_first[r]: the piece [s, ...) is kept

// ev[i] = key of reference row i's start, ev[n + i] = key of its end (rows of a bad chromosome id -- an error
// the span pass has flagged -- get key 0) + the 4 x 256 digit histogram of the 2n keys, as k_linearize counts it.
__global__ __launch_bounds__(LIN_NT) void k_dj_events(SideView r, int n_chrom, const i64* __restrict__ chrom_base,
                                                      u32* __restrict__ ev, u32* __restrict__ hist_partial,
                                                      DevMeta* __restrict__ meta, u32 bad_bit) {
  __shared__ u32 s_hist[4 * 256];
  for (int k = threadIdx.x; k < 4 * 256; k += LIN_NT) s_hist[k] = 0;
  __syncthreads();
  const u32 stride = gridDim.x * LIN_NT;
  bool bad = false;
  for (u32 i = blockIdx.x * LIN_NT + threadIdx.x; i < r.n; i += stride) {
    const int c = r.chrom[i];
    const i64 cs = (i64)r.start[i] + r.start_off, ce = (i64)r.end[i] + r.end_off;
    u32 ks = 0, ke = 0;
    if (c >= 0 && c < n_chrom) {
      if (ce < cs) {
        bad = true;
      } else {
        const i64 b = chrom_base[c];
        ks = (u32)(b + cs);
        ke = (u32)(b + ce);
      }
    }
    ev[i] = ks;
    ev[r.n + i] = ke;
#pragma unroll
    for (int p = 0; p < 4; p++) {
      atomicAdd(&s_hist[p * 256 + ((ks >> (8 * p)) & 0xFFu)], 1u);
      atomicAdd(&s_hist[p * 256 + ((ke >> (8 * p)) & 0xFFu)], 1u);
    }
  }
  if (__ballot(bad) != 0ull && lane_id() == 0) atomicOr(&meta->aux0, bad_bit);
  __syncthreads();
  u32* g = hist_partial + (size_t)(blockIdx.x % LIN_HIST_REPLICAS) * 1024;
  for (int k = threadIdx.x; k < 4 * 256; k += LIN_NT) {
    const u32 v = s_hist[k];
    if (v) atomicAdd(&g[k], v);
  }
}

// over the sorted events: last[i] = 1 at the last event of a run of equal keys, is_start[i] = the event is a start
__global__ __launch_bounds__(256) void k_dj_flags(const u32* __restrict__ keys, const u32* __restrict__ rids, u32 n_ev,
                                                  u32 n_ref, u32* __restrict__ last, u32* __restrict__ is_start) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_ev) return;
  last[i] = (i + 1 == n_ev || keys[i + 1] != keys[i]) ? 1u : 0u;
  is_start[i] = rids[i] < n_ref ? 1u : 0u;
}

// bp[u] = the u-th distinct key; cov[u] = 1 when a reference row covers [bp[u], bp[u] + 1) (cov == NULL: self mode)
__global__ __launch_bounds__(256) void k_dj_compact(const u32* __restrict__ keys, const u32* __restrict__ last,
                                                    const u32* __restrict__ last_excl, const u32* __restrict__ is_start,
                                                    const u32* __restrict__ start_excl, u32 n_ev, u32* __restrict__ bp,
                                                    u32* __restrict__ cov) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_ev || !last[i]) return;
  const u32 u = last_excl[i];
  bp[u] = keys[i];
  if (cov) cov[u] = 2ull * (start_excl[i] + is_start[i]) > (u64)i + 1 ? 1u : 0u;
}

// cbp[j] = index of the j-th covered breakpoint (cov is zero past the last breakpoint)
__global__ __launch_bounds__(256) void k_dj_covered(const u32* __restrict__ cov, const u32* __restrict__ ncov, u32 n_ev,
                                                    u32* __restrict__ cbp) {
  const u32 u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u < n_ev && cov[u]) cbp[ncov[u]] = u;
}

// per target row (input order): the number of pieces it leaves and where they begin in bp
__global__ __launch_bounds__(256) void k_dj_count(SideView t, int n_chrom, const i64* __restrict__ chrom_base,
                                                  const u32* __restrict__ bp, const u64* __restrict__ n_bp,
                                                  const u32* __restrict__ cov, const u32* __restrict__ ncov,
                                                  u32* __restrict__ cnt, u32* __restrict__ lo_first,
                                                  DevMeta* __restrict__ meta) {
  const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= t.n) return;
  const int c = t.chrom[r];
  const i64 cs = (i64)t.start[r] + t.start_off, ce = (i64)t.end[r] + t.end_off;
  u32 count = 0, lf = 0;
  if (c >= 0 && c < n_chrom) {
    if (ce < cs) {
      atomicOr(&meta->aux0, DJ_BAD_TARGET);
    } else if (cs < ce) {
      const u32 U = (u32)*n_bp;
      const i64 b = chrom_base[c];
      const u32 ks = (u32)(b + cs), ke = (u32)(b + ce);
      const u32 lo = upper_bound_u32(bp, 0, U, ks);
      const u32 hi = lower_bound_u32(bp, lo, U, ke);
      if (cov) {
        const u32 first = (lo > 0 && cov[lo - 1]) ? 1u : 0u;
        count = first + ncov[hi] - ncov[lo];
        lf = lo | (first ? DJ_FIRST : 0u);
      } else {
        count = hi - lo + 1;
        lf = lo | DJ_FIRST;
      }
    }
  }
  cnt[r] = count;
  lo_first[r] = lf;
}

constexpr int DJ_FILL_NT = 256;
constexpr int DJ_FILL_ITEMS = 4;                          // consecutive output slots per thread: one 16-byte store per array
constexpr u32 DJ_FILL_TILE = DJ_FILL_NT * DJ_FILL_ITEMS;  // output slots per block
constexpr u32 DJ_OFF_CAP = 4096;                          // parent rows of a tile staged in LDS (16 KB)

struct DjPiece {
  int parent, start, end;
};

// slot k (of parent row r) -> its piece, in the target's declared encoding
__device__ __forceinline__ DjPiece dj_piece(const SideView& t, const i64* __restrict__ chrom_base, u32 r, u32 j,
                                            const u32* __restrict__ lo_first, const u32* __restrict__ bp, u32 U,
                                            const u32* __restrict__ ncov, const u32* __restrict__ cbp) {
  const i64 b = chrom_base[t.chrom[r]];
  const u32 ks = (u32)(b + t.start[r] + t.start_off), ke = (u32)(b + t.end[r] + t.end_off);
  const u32 lf = lo_first[r];
  const u32 lo = lf & ~DJ_FIRST, first = lf >> 31;
  u32 ps, nx;
  if (first && j == 0) {
    ps = ks;
    nx = lo;
  } else {
    const u32 u = cbp ? cbp[ncov[lo] + (j - first)] : lo + j - 1;
    ps = bp[u];
    nx = u + 1;
  }
  u32 pe = ke;
  if (nx < U) {
    const u32 q = bp[nx];
    pe = q < ke ? q : ke;
  }
  DjPiece p;
  p.parent = (int)r;
  p.start = (int)((i64)ps - b - t.start_off);
  p.end = (int)((i64)pe - b - t.end_off);
  return p;
}

// off: exclusive int64 offsets of the rows' counts; total = their sum.  vec: the three outputs are 16-byte aligned.
__global__ __launch_bounds__(DJ_FILL_NT) void k_dj_fill(SideView t, const i64* __restrict__ chrom_base,
                                                        const u64* __restrict__ off, u64 total,
                                                        const u32* __restrict__ lo_first, const u32* __restrict__ bp,
                                                        const u64* __restrict__ n_bp, const u32* __restrict__ ncov,
                                                        const u32* __restrict__ cbp, int vec, int* __restrict__ parent,
                                                        int* __restrict__ dstart, int* __restrict__ dend) {
  __shared__ u32 s_rel[DJ_OFF_CAP];
  __shared__ u32 s_rows[2];
  const u64 k0 = (u64)blockIdx.x * DJ_FILL_TILE;
  if (k0 >= total) return;
  const u64 k1 = k0 + DJ_FILL_TILE < total ? k0 + DJ_FILL_TILE : total;
  // the tile's first and last parent row: the last row whose offset is <= the slot (rows without pieces share
  // their successor's offset and are never that row)
  if (threadIdx.x < 2) s_rows[threadIdx.x] = (u32)(upper_bound_u64(off, 0, t.n, threadIdx.x ? k1 - 1 : k0) - 1);
  __syncthreads();
  const u32 r_lo = s_rows[0], nr = s_rows[1] - r_lo + 1;
  const bool staged = nr <= DJ_OFF_CAP;
  if (staged)
    for (u32 j = threadIdx.x; j < nr; j += DJ_FILL_NT) {
      const u64 o = off[r_lo + j];
      s_rel[j] = o <= k0 ? 0u : (u32)(o - k0);
    }
  __syncthreads();
  const u32 U = (u32)*n_bp;
  const u64 kt = k0 + (u64)threadIdx.x * DJ_FILL_ITEMS;
  DjPiece p[DJ_FILL_ITEMS];
#pragma unroll
  for (int i = 0; i < DJ_FILL_ITEMS; i++) {
    const u64 k = kt + i;
    if (k >= k1) break;
    const u32 r = staged ? r_lo + upper_bound_u32(s_rel, 0, nr, (u32)(k - k0)) - 1
                         : (u32)(upper_bound_u64(off, r_lo, (u64)r_lo + nr, k) - 1);
    p[i] = dj_piece(t, chrom_base, r, (u32)(k - off[r]), lo_first, bp, U, ncov, cbp);
  }
  if (vec && kt + DJ_FILL_ITEMS <= k1) {
    *reinterpret_cast<int4*>(parent + kt) = make_int4(p[0].parent, p[1].parent, p[2].parent, p[3].parent);
    *reinterpret_cast<int4*>(dstart + kt) = make_int4(p[0].start, p[1].start, p[2].start, p[3].start);
    *reinterpret_cast<int4*>(dend + kt) = make_int4(p[0].end, p[1].end, p[2].end, p[3].end);
  } else {
#pragma unroll
    for (int i = 0; i < DJ_FILL_ITEMS; i++) {
      if (kt + i >= k1) break;
      parent[kt + i] = p[i].parent;
      dstart[kt + i] = p[i].start;
      dend[kt + i] = p[i].end;
    }
  }
}

}  // namespace giql
