// string_agg_kernels.hip.h -- STRING_AGG beside MERGE (bedtools `merge -c 4 -o collapse`): per merged region the
// region's non-NULL names joined by a separator, in the sorted order of cluster_front (ascending start, then row id).
//
// After cluster_front a region is a contiguous run of the sorted order, so the variable-length output is three exclusive
// scans away.  With c_i = valid ? sep_len + len : 0 and v_i = valid per sorted position i:
//   G = scan(c) (64-bit), V = scan(v);  region g = [h_g, h_g+1):  nn_g = V[h_g+1] - V[h_g],
//   bytes_g = G[h_g+1] - G[h_g] - (nn_g ? sep_len : 0)   (every value brings a separator but the region's first),
//   out_offsets = scan(bytes_g);  value i starts at out_offsets[g] + G[i] - G[h_g], its separator sits in front of it
//   iff V[i] > V[h_g].
//   k_sagg_len      the one random gather of the plan: offsets[rid], offsets[rid + 1], valid[rid] -> c, v (+ the order)
//   k_sagg_regions  per region: byte count (clamped so the scan's 64-bit total shows an overflow) and out_nn
//   k_sagg_rows     per sorted position: row_dst; the region heads copy out_offsets
//   k_sagg_fill     the bytes, modelled on k_take_utf8_copy: one lane per row for short values, so adjacent lanes write
//                   adjacent bytes; the whole wave for long ones; a separator is written by the lane (wave) that owns
//                   the value behind it.  Every output byte has exactly one writer.
// No atomics: the two error flags are plain stores of one constant (every writer stores the same value).
#pragma once
#include "dev_common.hip.h"
#include "take_kernels.hip.h"  // TKS_SHORT, TkU128, shfl_u64

namespace giql {

constexpr int SAGG_NT = 256;
constexpr int SAGG_MAX = 4;        // = GIQL_STR_AGG_MAX
constexpr int SAGG_SEP_MAX = 255;  // = GIQL_STR_AGG_MAX_SEP
constexpr u32 SAGG_NULL = 0xFFFFFFFFu;
constexpr u32 SAGG_SEP_BIT = 0x80000000u;
constexpr u32 SAGG_SEP_LANE = 16;  // a separator up to this long is written by the value's own lane

struct SaggSep {
  u32 len;
  unsigned char b[SAGG_SEP_MAX + 1];
};

// rids: the sorted order (each < n: the sort's own ids).  bad: one zeroed word.
__global__ __launch_bounds__(SAGG_NT) void k_sagg_len(const u32* __restrict__ rids, u32 n,
                                                      const int* __restrict__ offsets,
                                                      const unsigned char* __restrict__ valid, u32 sep_len,
                                                      u32* __restrict__ c, u32* __restrict__ v,
                                                      int* __restrict__ out_order, u32* __restrict__ bad) {
  const u32 i = blockIdx.x * SAGG_NT + threadIdx.x;
  if (i >= n) return;
  const u32 r = rids[i];
  if (out_order) out_order[i] = (int)r;
  bool ok = r < n && (!valid || valid[r] != 0);
  u32 len = 0;
  if (ok) {
    const int lo = offsets[r], hi = offsets[r + 1];
    if (lo < 0 || hi < lo) {
      *bad = 1u;
      ok = false;
    } else {
      len = (u32)(hi - lo);
    }
  }
  c[i] = ok ? sep_len + len : 0u;  // (< 2^31 + 256)
  v[i] = ok ? 1u : 0u;
}

// G[n] is the scan's total (written by the spine); V's total arrives in *v_total
__global__ __launch_bounds__(SAGG_NT) void k_sagg_regions(const u32* __restrict__ head_pos, u32 m, u32 n,
                                                          const u64* __restrict__ G, const u32* __restrict__ V,
                                                          const u64* __restrict__ v_total, u32 sep_len,
                                                          u32* __restrict__ bytes, i64* __restrict__ out_nn) {
  const u32 g = blockIdx.x * SAGG_NT + threadIdx.x;
  if (g >= m) return;
  const u32 h0 = head_pos[g];
  const u32 h1 = g + 1 < m ? head_pos[g + 1] : n;
  const u32 nn = (h1 < n ? V[h1] : (u32)*v_total) - V[h0];
  const u64 b = G[h1] - G[h0] - (nn ? sep_len : 0u);
  bytes[g] = b > 0x7FFFFFFFull ? 0x80000000u : (u32)b;  // (a clamped region alone carries the total past 2^31 - 1)
  out_nn[g] = (i64)nn;
}

// roff: the exclusive scan of `bytes`, r_total its total.  When the total does not fit, row_dst is not meaningful
// (the host reports GIQL_ERR_CAPACITY); nothing is addressed through it here.
__global__ __launch_bounds__(SAGG_NT) void k_sagg_rows(const u32* __restrict__ excl, const u32* __restrict__ flags,
                                                       const u32* __restrict__ head_pos, u32 n, u32 m,
                                                       const u64* __restrict__ G, const u32* __restrict__ V,
                                                       const u32* __restrict__ v, const u32* __restrict__ roff,
                                                       const u64* __restrict__ r_total, int* __restrict__ out_offsets,
                                                       u32* __restrict__ row_dst) {
  const u32 i = blockIdx.x * SAGG_NT + threadIdx.x;
  if (i >= n) return;
  const u32 g = excl[i] + flags[i] - 1u;  // (every partition's first row is a head)
  if (g >= m) return;                      // (cannot happen: m is the scan's total)
  const u32 h = head_pos[g];
  const u32 o = roff[g];
  if (flags[i]) out_offsets[g] = (int)o;
  if (i == 0) out_offsets[m] = (int)(*r_total > 0x7FFFFFFFull ? 0x7FFFFFFFull : *r_total);
  u32 d = SAGG_NULL;
  if (v[i]) d = ((u32)((u64)o + (G[i] - G[h])) & ~SAGG_SEP_BIT) | (V[i] > V[h] ? SAGG_SEP_BIT : 0u);
  row_dst[i] = d;
}

__global__ __launch_bounds__(SAGG_NT) void k_sagg_fill(const int* __restrict__ offsets,
                                                       const uint8_t* __restrict__ data, u32 n_rows,
                                                       const int* __restrict__ order,
                                                       const u32* __restrict__ row_dst, u64 n, SaggSep sep,
                                                       uint8_t* __restrict__ out, int* __restrict__ status) {
  __shared__ uint8_t s_sep[SAGG_SEP_MAX + 1];
  if (threadIdx.x < sep.len) s_sep[threadIdx.x] = sep.b[threadIdx.x];
  __syncthreads();
  const u64 stride = (u64)gridDim.x * SAGG_NT;
  const u64 n_pad = (n + 63) & ~(u64)63;  // whole waves stay in the loop together
  bool bad = false;
  for (u64 i = (u64)blockIdx.x * SAGG_NT + threadIdx.x; i < n_pad; i += stride) {
    u32 len = 0, sl = 0;
    bool live = false;
    const uint8_t* src = data;
    uint8_t* dst = out;
    if (i < n) {
      const u32 d = row_dst[i];
      if (d != SAGG_NULL) {
        const u32 r = (u32)order[i];
        const u32 at = d & ~SAGG_SEP_BIT;
        const u32 want = (d & SAGG_SEP_BIT) ? sep.len : 0u;
        if (r >= n_rows || at < want) {
          bad = true;
        } else {
          const int lo = offsets[r], hi = offsets[r + 1];
          if (lo < 0 || hi < lo) {
            bad = true;
          } else {
            live = true;
            len = (u32)(hi - lo);
            sl = want;
            src = data + lo;
            dst = out + at;
          }
        }
      }
    }
    const bool is_long = live && (len > TKS_SHORT || sl > SAGG_SEP_LANE);
    const u32 slen = is_long ? 0u : len;
    if (!is_long)
      for (u32 k = 0; k < sl; k++) (dst - sl)[k] = s_sep[k];
    // short values: 16 / 8 / 4-byte pieces at the value's own alignment, then at most 3 single bytes (k_take_utf8_copy)
    {
      u32 k = 0;
      for (; k + 16 <= slen; k += 16) {
        TkU128 w;
        __builtin_memcpy(&w, src + k, 16);
        __builtin_memcpy(dst + k, &w, 16);
      }
      if (k + 8 <= slen) {
        u64 w;
        __builtin_memcpy(&w, src + k, 8);
        __builtin_memcpy(dst + k, &w, 8);
        k += 8;
      }
      if (k + 4 <= slen) {
        u32 w;
        __builtin_memcpy(&w, src + k, 4);
        __builtin_memcpy(dst + k, &w, 4);
        k += 4;
      }
      for (; k < slen; k++) dst[k] = src[k];
    }
    u64 longs = __ballot(is_long);
    while (longs) {
      const int l = __ffsll((long long)longs) - 1;
      longs &= longs - 1;
      const u64 s = shfl_u64((u64)(uintptr_t)src, l);
      const u64 d = shfl_u64((u64)(uintptr_t)dst, l);
      const u32 ln = (u32)__shfl((int)len, l, 64);
      const u32 wsl = (u32)__shfl((int)sl, l, 64);
      const uint8_t* ws = reinterpret_cast<const uint8_t*>((uintptr_t)s);
      uint8_t* wd = reinterpret_cast<uint8_t*>((uintptr_t)d);
      for (u32 k = lane_id(); k < wsl; k += WAVE) (wd - wsl)[k] = s_sep[k];
      // 4 bytes per lane per step (unaligned dwords), then the last ln % 4 bytes
      const u32 body = ln & ~3u;
      for (u32 k = lane_id() * 4u; k < body; k += 256u) {
        u32 w;
        __builtin_memcpy(&w, ws + k, 4);
        __builtin_memcpy(wd + k, &w, 4);
      }
      if (lane_id() < (ln & 3u)) wd[body + lane_id()] = ws[body + lane_id()];
    }
  }
  if (bad) *status = -1;  // GIQL_ERR_INVALID
}

}  // namespace giql
