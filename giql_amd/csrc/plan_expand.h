// giql_amd/csrc/plan_expand.h -- host threads expand a compact join plan into its pairs while its sorted ids still
// arrive: the second half of giql_hip_inner's compact-plan download (giql_hip.hip: inner_host_compact_tail).  Plain
// C++17, no HIP: the caller hands in how to wait for a chunk (tests/native/host_side_check.cpp: without a GPU).
#pragma once

#include <atomic>
#include <cstdint>
#include <thread>
#include <vector>
#if defined(__SSE2__)
#include <emmintrin.h>
#endif

#include "../../include/giql_hip.h"

struct CompactPlan {  // the host arrays of a compact plan: nq queries {row id, first match, count}, ns sorted row ids
  const int32_t* q_rid;
  const uint32_t *lo, *cnt;
  const int32_t* s_rid;
  size_t nq, ns;
};

// the pairs of queries [q0, q1), from output index o on: plain stores
static inline void expand_block_plain(const int32_t* q_rid, const uint32_t* lo, const uint32_t* cnt, const int32_t* s_rid,
                                      size_t q0, size_t q1, uint64_t o, int32_t* out_q, int32_t* out_s) {
  for (size_t q = q0; q < q1; q++) {
    const uint32_t c = cnt[q];
    const int32_t id = q_rid[q];
    const int32_t* src = s_rid + lo[q];
    for (uint32_t k = 0; k < c; k++) {
      out_q[o + k] = id;
      out_s[o + k] = src[k];
    }
    o += c;
  }
}

#if defined(__SSE2__)
// The pairs [o, o_end) of the block that starts at query q0.  They are staged in two 4 KB buffers (L1) and leave in
// aligned 16-byte NON-TEMPORAL stores: a plain store makes the core read every output line before writing it, i.e.
// 6.4 GB of memory traffic for 3.2 GB of pairs.  Both arrays are 64-byte aligned, so one alignment serves both.
static inline void expand_block_streamed(const int32_t* q_rid, const uint32_t* lo, const uint32_t* cnt, const int32_t* s_rid,
                                         size_t q0, uint64_t o, uint64_t o_end, int32_t* out_q, int32_t* out_s) {
  constexpr uint32_t BUF = 1024;
  alignas(64) int32_t bq[BUF], bs[BUF];
  size_t q = q0;
  uint32_t k = 0;  // next pair of query q
  auto next_pair = [&](int32_t& vq, int32_t& vs) {  // (the block holds o_end - o more pairs: never runs past its queries)
    while (k >= cnt[q]) q++, k = 0;
    vq = q_rid[q];
    vs = s_rid[lo[q] + k];
    k++;
  };
  while (o < o_end && (o & 15u)) {  // up to the first 64-byte boundary: plain stores
    next_pair(out_q[o], out_s[o]);
    o++;
  }
  while (o_end - o >= BUF) {
    uint32_t f = 0;
    while (f < BUF) {  // whole runs of one query at a time
      while (k >= cnt[q]) q++, k = 0;
      const uint32_t c = cnt[q] - k < BUF - f ? cnt[q] - k : BUF - f;
      const int32_t id = q_rid[q];
      const int32_t* src = s_rid + lo[q] + k;
      for (uint32_t j = 0; j < c; j++) {
        bq[f + j] = id;
        bs[f + j] = src[j];
      }
      f += c;
      k += c;
    }
    for (uint32_t j = 0; j < BUF; j += 4) {
      _mm_stream_si128(reinterpret_cast<__m128i*>(out_q + o + j), _mm_load_si128(reinterpret_cast<const __m128i*>(bq + j)));
      _mm_stream_si128(reinterpret_cast<__m128i*>(out_s + o + j), _mm_load_si128(reinterpret_cast<const __m128i*>(bs + j)));
    }
    o += BUF;
  }
  while (o < o_end) {
    next_pair(out_q[o], out_s[o]);
    o++;
  }
  _mm_sfence();
}
#endif

// Writes the pairs of the plan in query order: out_q[i] = q_rid[q], out_s[i] = s_rid[lo[q] + k] for k < cnt[q].  The
// per-query arrays are in memory; the sorted ids arrive in chunks of `chunk_ids`: wait_chunk(c) blocks until chunk c is
// there and returns non-zero when it never will be.  Blocks of `blk_queries` queries are handed out in order to `n_thr`
// threads (and to this one, once every chunk is there); a block waits for the chunk that holds its furthest id.
// PRECONDITION: out_q and out_s hold n_pairs entries each and are both 64-byte aligned (a block's non-temporal stores
// start at the same index of both).
// Returns GIQL_OK or what fail(code, format, ...) returns (set_err); after GIQL_ERR_STATE nothing has been written.
template <typename WaitChunk>
static int expand_plan(const CompactPlan& p, uint64_t n_pairs, int32_t* out_q, int32_t* out_s, int n_thr, bool stream_stores,
                       size_t chunk_ids, size_t blk_queries, WaitChunk wait_chunk, int (*fail)(int, const char*, ...)) {
  const size_t n_chunks = (p.ns + chunk_ids - 1) / chunk_ids, n_blk = (p.nq + blk_queries - 1) / blk_queries;
  if ((size_t)n_thr > n_blk) n_thr = (int)n_blk;
  if (n_thr < 1) n_thr = 1;
  // block offsets: per-block sums in parallel, a serial scan over the (few hundred) blocks
  std::vector<uint64_t> blk_off(n_blk + 1, 0);
  std::vector<uint32_t> blk_need(n_blk, 0);  // one past the last sorted id a block reads
  std::atomic<size_t> next{0};
  std::atomic<size_t> chunks_here{0};
  std::atomic<int> bad{0};
  auto sums = [&] {
    for (size_t bk; (bk = next.fetch_add(1)) < n_blk;) {
      const size_t q0 = bk * blk_queries, q1 = q0 + blk_queries < p.nq ? q0 + blk_queries : p.nq;
      uint64_t t = 0;
      uint32_t need_s = 0;
      for (size_t q = q0; q < q1; q++) {
        t += p.cnt[q];
        const uint64_t e = (uint64_t)p.lo[q] + p.cnt[q];
        if (p.cnt[q] && e > need_s) need_s = e > (uint64_t)p.ns ? 0xFFFFFFFFu : (uint32_t)e;
      }
      blk_off[bk + 1] = t;
      blk_need[bk] = need_s;
    }
  };
  {
    std::vector<std::thread> th;
    try {
      for (int t = 1; t < n_thr; t++) th.emplace_back(sums);
    } catch (...) {  // no more threads to be had: the ones that started (and this one) do the work
    }
    sums();
    for (auto& t : th) t.join();
  }
  for (size_t bk = 0; bk < n_blk; bk++) {
    if (blk_need[bk] == 0xFFFFFFFFu) return fail(GIQL_ERR_STATE, "compact plan: a range past the sorted ids");
    blk_off[bk + 1] += blk_off[bk];
  }
  if (blk_off[n_blk] != n_pairs)
    return fail(GIQL_ERR_STATE, "compact plan: %llu pairs, the plan counted %lld", (unsigned long long)blk_off[n_blk], (long long)n_pairs);
  next.store(0);
  auto expand = [&] {
    for (size_t bk; (bk = next.fetch_add(1)) < n_blk;) {
      const size_t want = ((size_t)blk_need[bk] + chunk_ids - 1) / chunk_ids;  // chunks that must have arrived
      while (chunks_here.load(std::memory_order_acquire) < want) {
        if (bad.load()) return;
        std::this_thread::yield();
      }
      const size_t q0 = bk * blk_queries, q1 = q0 + blk_queries < p.nq ? q0 + blk_queries : p.nq;
#if defined(__SSE2__)
      if (stream_stores) {
        expand_block_streamed(p.q_rid, p.lo, p.cnt, p.s_rid, q0, blk_off[bk], blk_off[bk + 1], out_q, out_s);
        continue;
      }
#endif
      expand_block_plain(p.q_rid, p.lo, p.cnt, p.s_rid, q0, q1, blk_off[bk], out_q, out_s);
    }
  };
  std::vector<std::thread> th;
  try {
    for (int t = 0; t < n_thr; t++) th.emplace_back(expand);
  } catch (...) {  // (as above; this thread expands too once every chunk has arrived)
  }
  int rc = GIQL_OK;
  for (size_t c = 0; c < n_chunks; c++) {  // this thread follows the chunks and publishes what has arrived
    if (wait_chunk(c) != 0) {
      rc = fail(GIQL_ERR_HIP, "D2H copy of the compact plan failed");
      bad.store(1);
      break;
    }
    chunks_here.store(c + 1, std::memory_order_release);
  }
  if (rc == GIQL_OK) expand();  // whatever blocks are left (all of them when no helper thread could be started)
  for (auto& t : th) t.join();
  return rc;
}
