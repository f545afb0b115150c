// tests/native/sort_plan_check.cpp -- giql_amd/csrc/sort_plan.h checked without a GPU.
//
//   g++ -std=c++17 -O1 -o sort_plan_check tests/native/sort_plan_check.cpp && ./sort_plan_check
//   (the same with -fsanitize=address,undefined, by hand)
//
// Two kinds of checks, over one grid of tunings and requests:
//   1. plan_sort and every decision function against the REFERENCE below: a literal transcription of the arithmetic the
//      host driver held inline before the plan existed;
//   2. properties that hold in their own right (digits, buffers, status words, what the span pass has to count).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <vector>

#include "../../giql_amd/csrc/sort_plan.h"

using namespace giql;
typedef uint32_t u32;
typedef uint64_t u64;

static long g_checked = 0;
#define REQUIRE(cond, ...)                                   \
  do {                                                       \
    if (!(cond)) {                                           \
      printf("FAIL %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
      printf(__VA_ARGS__);                                   \
      printf("\n");                                          \
      exit(1);                                               \
    }                                                        \
  } while (0)

// ------------------------------------------------------------------------------------------------ the reference
// TRANSCRIPTION of giql_amd/csrc/giql_hip.hip at commit 07a39fdf3e38b3c438a12f6356862fc9b237ef00 (the parent of the
// change that introduced sort_plan.h): its lines 709-716, 749-781, 860-863, 869-925, 952-974 and 1129-1141, and the
// hist-mode expression of run_spans.  The context is restated as the three structs those lines read; launches are
// replaced by records of what would have been launched.  Nothing here includes or calls sort_plan.h.
namespace parent {
constexpr int OS_BINS = 256;
constexpr int OS_MIN_TILE = 4096;
constexpr int BS_MIN_WBITS = 13;
static inline u32 cdiv(u64 a, u64 b) { return (u32)((a + b - 1) / b); }

struct Ctx {
  struct {
    int os_variant = 0;
    bool no_coarse_b = false;
    double coarse_max_group_rows = 8.0;
    u64 local_min_rows = 1u << 21;
    double local_min_bucket_rows = 300.0;
    double local_max_bucket_rows = 2800.0;
    bool no_narrow = false;
    int force_bits = 0;
  } sw;
  struct {
    bool local_sort = true;
    u64 last_span = 0;
  } guess;
  struct {
    bool first_unstable = false;
    int force_local = 0;
    int index_bits = 16;
  } call;
  bool bucket_bnd = false;
};

// 709-716
static inline size_t os_pass_words(size_t n) { return (size_t)cdiv(n ? n : 1, OS_MIN_TILE) * OS_BINS + 16; }
static inline size_t os_pass_stride(const Ctx* ctx, size_t n) {
  return ctx->sw.os_variant == 0 ? (size_t)cdiv(n ? n : 1, 8192) * OS_BINS + 16 : os_pass_words(n);
}
// 749-781
static inline int density_bits(const Ctx* ctx, double per_bucket) {
  int w = 16;
  while (per_bucket > ctx->sw.local_max_bucket_rows && w > BS_MIN_WBITS && !ctx->sw.no_narrow) {
    per_bucket *= 0.5;
    w--;
  }
  return per_bucket <= ctx->sw.local_max_bucket_rows ? w : 0;
}
static inline int sort_local_bits(const Ctx* ctx, size_t n) {
  if (ctx->call.force_local > 0 && ctx->bucket_bnd && ctx->sw.os_variant == 0) return ctx->call.index_bits;
  if (ctx->call.force_local < 0) return 0;
  if (!(ctx->guess.local_sort && ctx->bucket_bnd && ctx->sw.os_variant == 0 && n >= ctx->sw.local_min_rows)) return 0;
  const double span = ctx->guess.last_span ? (double)ctx->guess.last_span : 3.2e9;
  double per_bucket = (double)n * 65536.0 / span;
  if (per_bucket < ctx->sw.local_min_bucket_rows) return 0;
  if (ctx->sw.force_bits) return ctx->sw.force_bits;
  return density_bits(ctx, per_bucket);
}
static inline bool sort_is_local(const Ctx* ctx, size_t n) { return sort_local_bits(ctx, n) != 0; }
static inline int local_passes(int wbits) { return wbits == 16 ? 2 : 3; }
// 1129-1141
static inline int row_skip(const Ctx* ctx, size_t nb) {
  if (ctx->guess.last_span == 0) return 1;
  return (double)nb * 65536.0 / (double)ctx->guess.last_span <= 1024.0 ? 2 : 1;
}
static inline bool coarse_b_ok(const Ctx* ctx, size_t nb) {
  if (ctx->sw.no_coarse_b || ctx->guess.last_span == 0 || sort_is_local(ctx, nb)) return false;
  return (double)nb * 256.0 / (double)ctx->guess.last_span <= ctx->sw.coarse_max_group_rows;
}
// run_spans: ms[k].hist = !with_hist ? 0 : (sort_local_bits(ctx, (size_t)s.n) == 16 ? 2 : 1)
static inline int span_hist(const Ctx* ctx, size_t n) { return sort_local_bits(ctx, n) == 16 ? 2 : 1; }

struct FuseCount {
  u32 nq_total;
  bool join, general;
};
// 860-863
static int64_t bucket_stage_fused_bytes(u32 n, const FuseCount& fuse) {
  if (fuse.general) return (int64_t)12 * n + (int64_t)12 * fuse.nq_total;
  return fuse.join ? (int64_t)8 * n + (int64_t)12 * fuse.nq_total : (int64_t)12 * n + (int64_t)16 * fuse.nq_total;
}

// what run_sort_onesweep did, as a record
struct Pass {
  int digit, src, dst, unstable;
  bool first, keygen;
  int64_t bytes;
};
struct Did {
  bool presorted = false;
  int stream = 0;  // 0 none, 1 k_keygen_stream<mode>, 2 k_iota
  int64_t stream_bytes = 0;
  int wbits = 0, n_pass = 0, first_digit = 0;
  Pass pass[4];
  bool swapped = false;  // the ping-pong pointers were exchanged: the result is in physical buffer 1
  size_t per_pass = 0, zeroed_words = 0;
  int stage = 0;  // 0 none, 1 plain, 2 fused
  int stage_fuse = 0, stage_payload = 0;
  int64_t stage_bytes = 0;
  bool last_sort_local = false;
};

// 869-925, 952-974.  rid0 / end0: sb.rid[0] / sb.end[0] non-NULL.
static Did run_sort_onesweep(const Ctx* ctx, bool rid0, bool end0, u32 n, bool keep_rids, bool keygen, int skip_digits,
                             const FuseCount* fuse, bool presorted) {
  Did d;
  if (presorted) {
    d.presorted = true;
    const int mode = (rid0 ? 1 : 0) | (end0 ? 2 : 0);
    const int wbits_pre = sort_local_bits(ctx, n);
    d.wbits = wbits_pre;
    const bool local_fused = fuse && mode == (fuse->general ? 3 : 1) && wbits_pre != 0;
    {
      if (keygen) {
        d.stream_bytes += (int64_t)4 * n * ((mode & 2 ? 3 : 2) + 1 + (mode & 1) + (mode & 2 ? 1 : 0));
        d.stream = 1;
      } else if (rid0 && !keep_rids) {
        d.stream_bytes += (int64_t)4 * n;
        d.stream = 2;
      }
    }
    if (!local_fused) return d;
    d.last_sort_local = true;
    d.stage = 2;  // launch_bucket_stage_fused(ctx, st, sb, n, gbase, *fuse, wbits_pre)
    d.stage_bytes = bucket_stage_fused_bytes(n, *fuse);
    d.stage_fuse = fuse->general ? 3 : (fuse->join ? 2 : 1);
    d.stage_payload = fuse->general ? 3 : 1;
    return d;
  }
  const int wbits = sort_local_bits(ctx, n);
  d.wbits = wbits;
  const bool local = wbits != 0;
  if (local) d.last_sort_local = true;
  if (local) skip_digits = 0;
  const int n_pass = local ? local_passes(wbits) : 4 - skip_digits;
  const int first_digit = local ? 4 - n_pass : skip_digits;
  const size_t per_pass = os_pass_stride(ctx, n);
  d.n_pass = n_pass, d.first_digit = first_digit, d.per_pass = per_pass;
  d.zeroed_words = n_pass * per_pass;  // take_zeroed(ctx, st, status, n_pass * per_pass * sizeof(u32))
  for (int pass = 0; pass < n_pass; pass++) {
    const int src = pass & 1, dst = src ^ 1;
    const int digit = first_digit + pass;
    const bool first = pass == 0 && !keep_rids;
    int64_t bytes;
    {
      const int w_out = 1 + (rid0 ? 1 : 0) + (end0 ? 1 : 0);
      const int w_in = (pass == 0 && keygen) ? 2 + (end0 ? 1 : 0) : 1 + ((rid0 && !first) ? 1 : 0) + (end0 ? 1 : 0);
      bytes = (int64_t)4 * (w_in + w_out) * n;
    }
    const int unstable = (pass == 0 && !keep_rids && ctx->call.first_unstable) ? 1 : 0;
    d.pass[pass] = {digit, src, dst, unstable, first, pass == 0 && keygen, bytes};
  }
  if (n_pass & 1) d.swapped = true;
  if (local) {
    const int mode = (rid0 ? 1 : 0) | (end0 ? 2 : 0);
    if (fuse && mode == (fuse->general ? 3 : 1)) {
      d.stage = 2;
      d.stage_bytes = bucket_stage_fused_bytes(n, *fuse);
      d.stage_fuse = fuse->general ? 3 : (fuse->join ? 2 : 1);
      d.stage_payload = fuse->general ? 3 : 1;
      return d;
    }
    d.stage = 1;
    d.stage_bytes = (int64_t)8 * (1 + (rid0 ? 1 : 0) + (end0 ? 1 : 0)) * n;
    d.stage_payload = mode;  // GIQL_BS_LAUNCH(mode)
  }
  return d;
}
}  // namespace parent

// ------------------------------------------------------------------------------------------------ the grid
static SortTuning tuning_of(const parent::Ctx& c) {
  SortTuning t;
  t.os_variant = c.sw.os_variant;
  t.local_min_rows = c.sw.local_min_rows;
  t.local_min_bucket_rows = c.sw.local_min_bucket_rows;
  t.local_max_bucket_rows = c.sw.local_max_bucket_rows;
  t.no_narrow = c.sw.no_narrow;
  t.force_bits = c.sw.force_bits;
  t.no_coarse_b = c.sw.no_coarse_b;
  t.coarse_max_group_rows = c.sw.coarse_max_group_rows;
  t.local_sort = c.guess.local_sort;
  t.last_span = c.guess.last_span;
  t.force_local = c.call.force_local;
  t.index_bits = c.call.index_bits;
  t.first_unstable = c.call.first_unstable;
  t.bucket_buffers = c.bucket_bnd;
  return t;
}

static std::vector<parent::Ctx> all_tunings() {
  std::vector<parent::Ctx> sw;
  {
    parent::Ctx c;  // defaults
    sw.push_back(c);
    parent::Ctx lifted = c;  // GIQL_HIP_LOCAL_MIN_ROWS=1 lifts the two density bounds (parse_local_min_rows)
    lifted.sw.local_min_rows = 1, lifted.sw.local_max_bucket_rows = 1e30, lifted.sw.local_min_bucket_rows = 0.0;
    sw.push_back(lifted);
    for (int bits : {13, 14, 15, 16})
      for (const parent::Ctx& base : {c, lifted}) {
        parent::Ctx f = base;
        f.sw.force_bits = bits;
        sw.push_back(f);
      }
    parent::Ctx nn = c;
    nn.sw.no_narrow = true;
    sw.push_back(nn);
    parent::Ctx v3 = c;
    v3.sw.os_variant = 3;
    sw.push_back(v3);
    parent::Ctx v3l = lifted;
    v3l.sw.os_variant = 3;
    sw.push_back(v3l);
    parent::Ctx nl = c;  // GIQL_HIP_NO_LOCAL_SORT=1 (or a context that gave the form up)
    nl.guess.local_sort = false;
    sw.push_back(nl);
  }
  std::vector<parent::Ctx> out;
  for (const parent::Ctx& s : sw)
    for (int force_local : {-1, 0, 1})
      for (int index_bits : {13, 16})
        for (bool buffers : {true, false})
          for (u64 span : {(u64)0, (u64)100000000, (u64)3200000000ull, (u64)0xFFFFFFFFull})
            for (bool unstable : {false, true}) {
              parent::Ctx c = s;
              c.call.force_local = force_local, c.call.index_bits = index_bits, c.bucket_bnd = buffers;
              c.guess.last_span = span, c.call.first_unstable = unstable;
              out.push_back(c);
            }
  return out;
}

static const u32 ROWS[] = {1, 8191, 8192, 8193, (1u << 21) - 1, 1u << 21, 100000000u, 1u << 30};
static const u32 NQ = 123457;  // query rows of a fused stage

static void check_decisions(const std::vector<parent::Ctx>& tunings) {
  for (const parent::Ctx& c : tunings) {
    const SortTuning t = tuning_of(c);
    for (u32 n : ROWS) {
      REQUIRE(sort_local_bits(t, n) == parent::sort_local_bits(&c, n), "n=%u", n);
      REQUIRE(sort_is_local(t, n) == parent::sort_is_local(&c, n), "n=%u", n);
      REQUIRE(row_skip(t, n) == parent::row_skip(&c, n), "n=%u", n);
      REQUIRE(coarse_b_ok(t, n) == parent::coarse_b_ok(&c, n), "n=%u", n);
      REQUIRE(os_pass_words(n) == parent::os_pass_words(n), "n=%u", n);
      REQUIRE(os_pass_stride(t, n) == parent::os_pass_stride(&c, n), "n=%u", n);
      REQUIRE(span_hist_mode(t, n) == parent::span_hist(&c, n), "n=%u", n);
      for (double per_bucket : {0.0, 299.0, 2800.0, 2800.5, 5600.0, 11200.0, 22400.0, 22401.0, 1e9, (double)n * 65536.0 / 3.2e9})
        REQUIRE(density_bits(t, per_bucket) == parent::density_bits(&c, per_bucket), "per_bucket=%f", per_bucket);
      g_checked += 8;
    }
    REQUIRE(os_pass_words(0) == parent::os_pass_words(0) && os_pass_stride(t, 0) == parent::os_pass_stride(&c, 0), "n=0");
  }
  for (int w : {13, 14, 15, 16}) REQUIRE(local_passes(w) == parent::local_passes(w), "w=%d", w);
  printf("ok   sort_plan: every decision function equals the transcription of the previous driver\n");
}

static void check_no_guess(const std::vector<parent::Ctx>& tunings) {
  for (const parent::Ctx& c : tunings) {
    if (c.guess.last_span != 0) continue;
    const SortTuning t = tuning_of(c);
    for (u32 n : ROWS) {
      REQUIRE(row_skip(t, n) == 1, "n=%u", n);
      REQUIRE(!coarse_b_ok(t, n), "n=%u", n);
    }
  }
  printf("ok   sort_plan: row_skip and coarse_b_ok give their no-guess answers before any call has run\n");
}

struct Request {
  u32 n;
  int payload;
  bool keep_rids, keygen, presorted;
  int skip_digits, fuse;
};

template <typename F>
static void for_each_request(const parent::Ctx& c, F&& f) {
  for (u32 n : ROWS)
    for (int payload = 0; payload < 4; payload++)
      for (bool keep_rids : {false, true})
        for (bool keygen : {false, true})
          for (int skip_digits : {0, 1, 2})
            for (bool presorted : {false, true})
              for (int fuse : {0, 1, 2, 3}) {
                // the driver cannot be asked for these:
                if (keygen && keep_rids) continue;  // a sort that keeps row ids is the second of two: its keys exist
                if (keygen && !presorted && !(payload & 1)) continue;  // the key-building PASS writes row ids (k_onesweep<1|3, .., KEYGEN>)
                if (keygen && !presorted && c.sw.os_variant != 0) continue;  // ... and exists in the default block shape only
                if (keep_rids && !(payload & 1)) continue;  // no rid array to keep
                f(Request{n, payload, keep_rids, keygen, presorted, skip_digits, fuse});
              }
}

static void check_plans(const std::vector<parent::Ctx>& tunings) {
  long plans = 0;
  for (const parent::Ctx& c : tunings) {
    const SortTuning t = tuning_of(c);
    for_each_request(c, [&](const Request& r) {
      parent::FuseCount fc{NQ, r.fuse == 2, r.fuse == 3};
      // (the general join's FuseCount may carry join = true as well: general wins, as in the driver)
      const parent::Did d = parent::run_sort_onesweep(&c, (r.payload & 1) != 0, (r.payload & 2) != 0, r.n, r.keep_rids,
                                                      r.keygen, r.skip_digits, r.fuse ? &fc : nullptr, r.presorted);
      SortOptions o;
      o.keep_rids = r.keep_rids, o.keygen = r.keygen, o.skip_digits = r.skip_digits, o.presorted = r.presorted;
      o.fuse = (SortFuse)r.fuse, o.fuse_queries = r.fuse ? NQ : 0;
      const SortPlan p = plan_sort(t, r.n, (SortPayload)r.payload, o);
#define SAME(a, b) REQUIRE((a) == (b), "n=%u payload=%d keep=%d keygen=%d skip=%d presorted=%d fuse=%d", r.n, r.payload, \
                           (int)r.keep_rids, (int)r.keygen, r.skip_digits, (int)r.presorted, r.fuse)
      SAME(p.presorted, d.presorted);
      SAME((int)p.stream, d.stream);
      SAME(p.stream_bytes, d.stream_bytes);
      SAME(p.wbits, d.wbits);
      SAME(p.n_pass, d.n_pass);
      SAME(p.first_digit, d.first_digit);
      SAME(p.result_buf, d.swapped ? 1 : 0);
      SAME(p.pass_stride, d.per_pass);
      SAME(p.status_words, d.zeroed_words);
      SAME((int)p.stage, d.stage);
      SAME(p.stage_fuse, d.stage_fuse);
      SAME(p.stage_payload, d.stage_payload);
      SAME(p.stage_bytes, d.stage_bytes);
      SAME(p.stage != BucketStage::NONE, d.last_sort_local);
      for (int k = 0; k < p.n_pass; k++) {
        SAME(p.pass[k].digit, d.pass[k].digit);
        SAME(p.pass[k].src, d.pass[k].src);
        SAME(p.pass[k].dst, d.pass[k].dst);
        SAME(p.pass[k].first, d.pass[k].first);
        SAME(p.pass[k].keygen, d.pass[k].keygen);
        SAME(p.pass[k].unstable ? 1 : 0, d.pass[k].unstable);
        SAME(p.pass[k].bytes, d.pass[k].bytes);
      }
      // the indexed join launches the fused stage alone: the same stage as a presorted sort's
      if (p.stage == BucketStage::FUSED) {
        const SortPlan f = plan_fused_stage(p.wbits, r.n, o.fuse, o.fuse_queries);
        SAME(f.stage_fuse, p.stage_fuse);
        SAME(f.stage_payload, p.stage_payload);
        SAME(f.stage_bytes, p.stage_bytes);
        SAME(f.n_pass, 0);
      }
#undef SAME
      plans++;
    });
  }
  g_checked += plans;
  printf("ok   sort_plan: every field of plan_sort equals the transcription of the previous driver (%ld plans)\n", plans);
}

static void check_properties(const std::vector<parent::Ctx>& tunings) {
  for (const parent::Ctx& c : tunings) {
    const SortTuning t = tuning_of(c);
    for_each_request(c, [&](const Request& r) {
      SortOptions o;
      o.keep_rids = r.keep_rids, o.keygen = r.keygen, o.skip_digits = r.skip_digits, o.presorted = r.presorted;
      o.fuse = (SortFuse)r.fuse, o.fuse_queries = r.fuse ? NQ : 0;
      const SortPlan p = plan_sort(t, r.n, (SortPayload)r.payload, o);
      REQUIRE(p.n_pass >= 0 && p.n_pass <= SORT_MAX_PASSES, "n_pass=%d", p.n_pass);
      if (r.presorted) {
        REQUIRE(p.n_pass == 0 && p.status_words == 0 && p.result_buf == 0, "a presorted side is not scattered");
        REQUIRE(p.stage != BucketStage::PLAIN, "the presorted form runs the bucket stage only as the carrier of a fused count");
      } else {
        REQUIRE(p.n_pass >= 2, "n_pass=%d", p.n_pass);
        for (int k = 0; k < p.n_pass; k++) {
          REQUIRE(p.pass[k].digit == p.first_digit + k, "digits are consecutive");
          REQUIRE(p.pass[k].src == (k & 1) && p.pass[k].dst == ((k & 1) ^ 1), "source and destination alternate from buffer 0");
          REQUIRE(k == 0 || (!p.pass[k].first && !p.pass[k].keygen && !p.pass[k].unstable), "only the first pass is special");
        }
        REQUIRE(p.pass[p.n_pass - 1].digit == 3, "the passes end at digit 3");
        REQUIRE(p.result_buf == (p.n_pass & 1), "the result ends in buffer n_pass & 1");
        REQUIRE(p.result_buf == p.pass[p.n_pass - 1].dst, "... which is where the last pass wrote");
        REQUIRE(p.status_words == (size_t)p.n_pass * os_pass_stride(t, r.n), "status words = passes x stride");
        REQUIRE(p.pass_stride <= os_pass_words(r.n), "a pass fits the words callers reserve for it");
        if (p.wbits != 0) REQUIRE(p.n_pass == local_passes(p.wbits) && p.stage != BucketStage::NONE, "three stages");
        else REQUIRE(p.n_pass == 4 - r.skip_digits && p.stage == BucketStage::NONE, "global passes only");
        // what the span pass counts for this side covers every digit its global passes scatter on
        const int mode = span_hist_mode(t, r.n);
        for (int k = 0; k < p.n_pass; k++)
          REQUIRE(mode == 1 || (mode == 2 && p.pass[k].digit >= 2), "span pass mode %d does not count digit %d", mode, p.pass[k].digit);
      }
      if (p.stage == BucketStage::FUSED)
        REQUIRE((int)r.payload == (r.fuse == 3 ? 3 : 1) && p.stage_fuse == r.fuse && p.wbits != 0, "a fused stage reads its own payload");
      if (p.stage == BucketStage::PLAIN) REQUIRE(p.stage_fuse == 0 && p.stage_payload == r.payload, "the plain stage");
      if (p.stage != BucketStage::NONE) REQUIRE(p.wbits >= SORT_MIN_WBITS && p.wbits <= 16, "wbits=%d", p.wbits);
    });
  }
  printf("ok   sort_plan: digits are consecutive and end at digit 3\n");
  printf("ok   sort_plan: source and destination alternate from buffer 0 and the result ends in buffer n_pass & 1\n");
  printf("ok   sort_plan: the status words zeroed are n_pass x stride\n");
  printf("ok   sort_plan: the span pass counts every digit the side's global passes scatter on, for every tuning\n");
  printf("ok   sort_plan: a three-stage sort ignores skip_digits; a fused stage only with its own payload; presorted runs only a fused stage\n");
}

int main() {
  const std::vector<parent::Ctx> tunings = all_tunings();
  check_decisions(tunings);
  check_no_guess(tunings);
  check_plans(tunings);
  check_properties(tunings);
  printf("%zu tunings, %ld comparisons\n", tunings.size(), g_checked);
  printf("all cases passed\n");
  return 0;
}
