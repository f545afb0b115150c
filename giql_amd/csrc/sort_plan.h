// giql_amd/csrc/sort_plan.h -- what a sort of the onesweep driver will do, decided before anything is launched.
// Plain C++17, no HIP and no context (tests/native/sort_plan_check.cpp: without a GPU).
//
// run_sort_onesweep (giql_hip.hip) builds ONE SortPlan per sort, zeroes the status words it names and launches the
// passes and the bucket stage it names; it decides nothing itself.  Everyone else who has to know what a sort of n
// rows will do -- the span pass (which digits to count), SideChain, the per-row operators, the index build (which
// buffer the rows end in) -- asks the functions below with the same SortTuning, so they cannot disagree with the sort.
#pragma once

#include <cstddef>
#include <cstdint>

namespace giql {

// The constants of the kernel headers the decisions read (giql_hip.hip asserts that they are the kernels' own).
constexpr int SORT_OS_BINS = 256;            // OS_BINS: digit values of a pass
constexpr int SORT_OS_MIN_TILE = 4096;       // OS_MIN_TILE: smallest tile of any instantiated onesweep variant
constexpr int SORT_OS_DEFAULT_TILE = 8192;   // rows of a tile of the default 1024 x 8 block shape
constexpr int SORT_MIN_WBITS = 13;           // BS_MIN_WBITS: key bits of the narrowest bucket
constexpr int SORT_MAX_PASSES = 4;

// Everything the decisions read of a context, by value: its switches, its guesses and the state of the call in
// flight (sort_tuning() in giql_hip.hip fills it).  Constant during a call, so every decision of one call agrees.
struct SortTuning {
  int os_variant = 0;                     // Switches: onesweep block shape (0: the default 1024 x 8)
  uint64_t local_min_rows = 1u << 21;
  double local_min_bucket_rows = 300.0;
  double local_max_bucket_rows = 2800.0;
  bool no_narrow = false;
  int force_bits = 0;
  bool no_coarse_b = false;
  double coarse_max_group_rows = 8.0;
  bool local_sort = true;                 // Guesses: the three-stage sort is still allowed on this context
  uint64_t last_span = 0;                 // ... linearised span of the context's last call (0: none has run)
  int force_local = 0;                    // CallState: +1 an index is being built, -1 global passes only
  int index_bits = 16;
  bool first_unstable = false;
  bool bucket_buffers = false;            // the context has the bucket stage's boundary / queue buffers
};

inline uint32_t sort_cdiv(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

// status words of ONE pass: a {flag,count} word per (tile, digit) + the ticket word
inline size_t os_pass_words(size_t n) {
  return (size_t)sort_cdiv(n ? n : 1, SORT_OS_MIN_TILE) * SORT_OS_BINS + 16;
}
// ... and what a pass of this context really uses (the default 1024 x 8 block shape has 8192-row tiles: half
// of the worst case, half the bytes to zero); the ticket word is the stride's 16th-last
inline size_t os_pass_stride(const SortTuning& t, size_t n) {
  return t.os_variant == 0 ? (size_t)sort_cdiv(n ? n : 1, SORT_OS_DEFAULT_TILE) * SORT_OS_BINS + 16 : os_pass_words(n);
}

// Sides of local_min_rows rows and more take the three-stage form: global passes on bits
// 16-23 and 24-31 only, then every 16-bit bucket sorted on its low bits inside LDS, in place
// (bucket_sort.hip.h) -- three trips through HBM instead of four.
// the narrowest-needed bucket for a table of per_bucket rows per 65,536 keys on average (0: too dense for any)
inline int density_bits(const SortTuning& t, double per_bucket) {
  int w = 16;
  while (per_bucket > t.local_max_bucket_rows && w > SORT_MIN_WBITS && !t.no_narrow) {
    per_bucket *= 0.5;
    w--;
  }
  return per_bucket <= t.local_max_bucket_rows ? w : 0;
}

// Returns 0 (four global passes) or the key bits of a bucket: 16 (two global passes), or 15 / 14 / 13 for denser
// tables (three global passes -- bits 8-15, 16-23, 24-31 -- and buckets of 2^W keys: bucket_sort.hip.h).
inline int sort_local_bits(const SortTuning& t, size_t n) {
  if (t.force_local > 0 && t.bucket_buffers && t.os_variant == 0) return t.index_bits;
  if (t.force_local < 0) return 0;
  if (!(t.local_sort && t.bucket_buffers && t.os_variant == 0 && n >= t.local_min_rows)) return 0;
  // The in-LDS stage holds 4096 rows per bucket; larger buckets go through a slow queue (one block each, two
  // more passes: 30M x 300M reads, ~6000 rows per bucket, spent 10.4 of 21 ms there).  So the form is taken
  // only while the AVERAGE bucket is comfortably below that -- by the span of the context's previous call
  // (a human-genome-sized axis until one has run); denser tables take the four global passes.  The value is
  // constant during a call (updated when it ends), so every decision of one call agrees.
  // Round 4: what decides is the DENSITY, not the row count -- a 12.5M-row shard of an 8-GPU run has the headline's
  // ~2,100 rows per bucket on an eighth of the axis and takes the same path (fused count, join in the bucket stage);
  // a 10M-row table over the whole genome (212 rows per bucket) does not: a block per bucket is mostly overhead there
  // (0.135 ms against 0.106 for the two passes it replaces).
  // Round 4, bucket width by density: past 2,800 rows per 65,536 keys (132M rows on a human-genome axis) the bucket
  // narrows -- 2^15, 2^14, 2^13 keys, up to ~1G rows -- instead of the form being given up.
  const double span = t.last_span ? (double)t.last_span : 3.2e9;
  double per_bucket = (double)n * 65536.0 / span;
  if (per_bucket < t.local_min_bucket_rows) return 0;
  if (t.force_bits) return t.force_bits;
  return density_bits(t, per_bucket);
}
inline bool sort_is_local(const SortTuning& t, size_t n) { return sort_local_bits(t, n) != 0; }
inline int local_passes(int wbits) { return wbits == 16 ? 2 : 3; }  // global passes before the bucket stage

// Which digits the span pass counts for a side whose keys it builds (k_chrom_minmax<HIST>): 1 = all four, 2 = digits
// 2 and 3 only (16-bit buckets: the low digits are sorted in LDS and not counted; narrower ones need the bits 8-15
// digit).  Every digit the side's global passes scatter on is among them (sort_plan_check.cpp holds that).
inline int span_hist_mode(const SortTuning& t, size_t n) { return sort_local_bits(t, n) == 16 ? 2 : 1; }

// Low digits the per-row operators leave unsorted on their QUERY side (its order only serves locality: the
// rows of a block should search neighbouring ranges of B).  One digit always; two (rows ordered by key >> 16
// only: two passes instead of three) when B is sparse enough that a 65536-key range of it -- what a block's
// bracket then covers at least -- still fits the LDS stage of k_nearest (cfg 5: 1.115 -> 1.063 ms).  The
// density comes from the span of the context's previous per-row call: a guess that only ever costs speed.
inline int row_skip(const SortTuning& t, size_t nb) {
  if (t.last_span == 0) return 1;
  return (double)nb * 65536.0 / (double)t.last_span <= 1024.0 ? 2 : 1;
}

// Fixed-length B of the per-row operators (SEMI / ANTI / COUNT): sorted without its lowest digit (three passes
// instead of four) when the rows sharing the upper 24 key bits are few enough to be looked at one by one
// (aux_kernels.hip.h, "sorted COARSELY") -- by the density of the context's previous call, like row_skip(): a guess
// that only costs speed.
inline bool coarse_b_ok(const SortTuning& t, size_t nb) {
  if (t.no_coarse_b || t.last_span == 0 || sort_is_local(t, nb)) return false;
  return (double)nb * 256.0 / (double)t.last_span <= t.coarse_max_group_rows;
}

// ------------------------------------------------------------------ one sort
// Which of the end / rid arrays travel with the keys: the kernels' MODE template argument, so the values are fixed.
enum class SortPayload { KEYS = 0, KEYS_RID = 1, KEYS_END = 2, KEYS_END_RID = 3 };
inline bool has_rid(SortPayload p) { return ((int)p & 1) != 0; }
inline bool has_end(SortPayload p) { return ((int)p & 2) != 0; }

// What the caller wants the bucket stage to answer on the way (bucket_sort.hip.h, FUSE): the range bounds of the
// fixed-length form's query rows, its whole join, or the two-class join of rows of any length.
enum class SortFuse { NONE = 0, BOUNDS = 1, JOIN = 2, GENERAL_JOIN = 3 };

struct SortOptions {
  bool keep_rids = false;   // the rid array already holds row ids (second sort of a two-key sort)
  bool keygen = false;      // the first pass builds the keys from the side's raw columns
  int skip_digits = 0;      // low digits left unsorted (global-passes form only)
  SortFuse fuse = SortFuse::NONE;
  uint32_t fuse_queries = 0;  // query rows of the fused stage (its bytes)
  bool presorted = false;   // the side arrives sorted: one streaming pass for what a sort would have left
};

enum class StreamKernel { NONE, KEYGEN, IOTA };  // the presorted form's one pass: k_keygen_stream<payload>, k_iota
enum class BucketStage { NONE, PLAIN, FUSED };

struct SortPass {
  int digit = 0;            // the pass scatters on key bits [8 digit, 8 digit + 8)
  int src = 0, dst = 0;     // physical buffers
  bool first = false;       // the row ids are synthesised (no rid array read)
  bool keygen = false;      // the keys are built from the raw columns (k_onesweep<.., KEYGEN>)
  bool unstable = false;    // rows of equal digits may leave in any order
  int64_t bytes = 0;        // algorithmic bytes: every array read + every array written, 4 B per row
};

struct SortPlan {
  bool presorted = false;
  StreamKernel stream = StreamKernel::NONE;  // presorted form only
  int64_t stream_bytes = 0;
  int wbits = 0;            // key bits of a bucket; 0: global passes only
  int n_pass = 0;           // global passes (0 in the presorted form)
  int first_digit = 0;
  SortPass pass[SORT_MAX_PASSES];
  int result_buf = 0;       // the physical buffer the sorted rows end in
  size_t pass_stride = 0;   // status words of one pass (the ticket word is the stride's 16th-last)
  size_t status_words = 0;  // ... of all passes: what the driver zeroes
  BucketStage stage = BucketStage::NONE;
  int stage_fuse = 0;       // k_bucket_sort<P, FUSE, ..>: FUSE
  int stage_payload = 0;    // ... and P
  int64_t stage_bytes = 0;
};

// The bucket stage of a fused sort, its algorithmic bytes up to the pairs (8 B each, added once the count is known):
// the rows' keys and ids read; bounds form: the ids written, the queries' keys and end keys read, two bounds each
// written; join form: the queries' keys, end keys and ids read; general form: (key, end, rid) of both sides read
inline int64_t bucket_stage_fused_bytes(uint32_t n, SortFuse fuse, uint32_t nq) {
  if (fuse == SortFuse::GENERAL_JOIN) return (int64_t)12 * n + (int64_t)12 * nq;
  return fuse == SortFuse::JOIN ? (int64_t)8 * n + (int64_t)12 * nq : (int64_t)12 * n + (int64_t)16 * nq;
}

// The fused bucket stage alone, over rows that are grouped by bucket already and stay so (a table index): no pass.
inline SortPlan plan_fused_stage(int wbits, uint32_t n, SortFuse fuse, uint32_t nq) {
  SortPlan p;
  p.presorted = true;
  p.wbits = wbits;
  p.stage = BucketStage::FUSED;
  p.stage_fuse = (int)fuse;
  p.stage_payload = fuse == SortFuse::GENERAL_JOIN ? 3 : 1;
  p.stage_bytes = bucket_stage_fused_bytes(n, fuse, nq);
  return p;
}

// The rules that hold whatever the caller asks for:
//   a three-stage sort ignores skip_digits (its global passes are the upper digits, all of them);
//   a fused stage is taken only when the payload is the one it reads -- (key, rid), or (key, end, rid) for the general
//     join -- and is otherwise the plain one;
//   the presorted form runs the bucket stage only as the carrier of a fused count.
inline SortPlan plan_sort(const SortTuning& t, uint32_t n, SortPayload payload, const SortOptions& o) {
  SortPlan p;
  const int rid = has_rid(payload) ? 1 : 0, end = has_end(payload) ? 1 : 0;
  p.wbits = sort_local_bits(t, n);
  const bool fused = o.fuse != SortFuse::NONE && p.wbits != 0 &&
                     payload == (o.fuse == SortFuse::GENERAL_JOIN ? SortPayload::KEYS_END_RID : SortPayload::KEYS_RID);
  p.presorted = o.presorted;
  if (o.presorted) {
    if (o.keygen) {  // chrom, start (and end) read; the key and every payload array written
      p.stream = StreamKernel::KEYGEN;
      p.stream_bytes = (int64_t)4 * n * ((end ? 3 : 2) + 1 + rid + end);
    } else if (rid && !o.keep_rids) {
      p.stream = StreamKernel::IOTA;
      p.stream_bytes = (int64_t)4 * n;
    }
  } else {
    const bool local = p.wbits != 0;
    p.n_pass = local ? local_passes(p.wbits) : 4 - o.skip_digits;
    p.first_digit = 4 - p.n_pass;
    p.pass_stride = os_pass_stride(t, n);
    p.status_words = (size_t)p.n_pass * p.pass_stride;
    for (int k = 0; k < p.n_pass; k++) {
      SortPass& s = p.pass[k];
      s.digit = p.first_digit + k;
      s.src = k & 1;
      s.dst = s.src ^ 1;
      s.first = k == 0 && !o.keep_rids;
      s.keygen = k == 0 && o.keygen;
      s.unstable = k == 0 && !o.keep_rids && t.first_unstable;
      // (KEYGEN reads chrom + start instead of the key; a first pass synthesises the row ids)
      const int w_out = 1 + rid + end;
      const int w_in = s.keygen ? 2 + end : 1 + ((rid && !s.first) ? 1 : 0) + end;
      s.bytes = (int64_t)4 * (w_in + w_out) * n;
    }
    p.result_buf = p.n_pass & 1;
    if (local) p.stage = BucketStage::PLAIN;
  }
  if (fused) {
    const SortPlan f = plan_fused_stage(p.wbits, n, o.fuse, o.fuse_queries);
    p.stage = f.stage, p.stage_fuse = f.stage_fuse, p.stage_payload = f.stage_payload, p.stage_bytes = f.stage_bytes;
  } else if (p.stage == BucketStage::PLAIN) {
    p.stage_payload = (int)payload;
    p.stage_bytes = (int64_t)8 * (1 + rid + end) * n;  // every array read once, written once
  }
  return p;
}

}  // namespace giql
