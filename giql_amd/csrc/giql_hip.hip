// giql_amd/csrc/giql_hip.hip -- C ABI of libgiql_hip.so (see include/giql_hip.h).
//
// Host-side orchestration only: arena carving, kernel launches on the caller's
// stream, one pinned-memory readback per join (the output size).  All arithmetic
// is in the *.hip.h kernels.  gfx950 only; there is no CPU fallback: without a
// HIP device every entry point fails with GIQL_ERR_HIP.
#include <hip/hip_runtime.h>
#include <chrono>
#include <initializer_list>
#include <memory>
#include <utility>
#include <thread>
#include <type_traits>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/giql_hip.h"
#include "../../include/giql_hip_range_sets.h"
#include "../../include/giql_hip_string_agg.h"
#include "../../include/giql_hip_pair_agg.h"
#include "../../include/giql_hip_pair_expr_agg.h"
#include "../../include/giql_hip_coverage.h"
#include "aux_kernels.hip.h"
#include "take_kernels.hip.h"
#include "select_kernels.hip.h"
#include "eval_kernels.hip.h"
#include "outer_kernels.hip.h"
#include "cluster_kernels.hip.h"
#include "merge_agg_kernels.hip.h"
#include "string_agg_kernels.hip.h"
#include "pair_agg_kernels.hip.h"
#include "pair_expr_agg_kernels.hip.h"
#include "range_set_kernels.hip.h"
#include "disjoin_kernels.hip.h"
#include "coverage_kernels.hip.h"
#include "contain_kernels.hip.h"
#include "distance_kernels.hip.h"
#include "row_pred_kernels.hip.h"
#include "dev_common.hip.h"
#include "join_kernels.hip.h"
#include "onesweep.hip.h"
#include "bucket_sort.hip.h"
#include "radix_sort.hip.h"
#include "scan.hip.h"
#include "probe_kernels.hip.h"
#include "index_rows_kernels.hip.h"
#include "index_nearest_kernels.hip.h"
#include "host_pool.h"
#include "plan_expand.h"
#include "zero_ledger.h"
#include "sort_plan.h"

using namespace giql;

// ------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";

static int set_err(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

#define HIP_TRY(expr)                                                                     \
  do {                                                                                    \
    hipError_t _e = (expr);                                                               \
    if (_e != hipSuccess)                                                                 \
      return set_err(GIQL_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                     __FILE__, __LINE__);                                                 \
  } while (0)

#define GIQL_TRY(expr)      \
  do {                      \
    int _rc = (expr);       \
    if (_rc != GIQL_OK) return _rc; \
  } while (0)

#include "owned_memory.h"  // (after set_err / HIP_TRY: its buffers report through them)

// tile shapes per class: class 1 = many queries with ~0.5 match each (B rows as
// queries), class 2 = fewer queries with tens of matches each (A rows)
#ifndef GIQL_RC_ITEMS
#define GIQL_RC_ITEMS 1
#endif
constexpr int RC_ITEMS_C2 = GIQL_RC_ITEMS;  // queries per thread of a count block
#ifndef GIQL_FILL_ITEMS
#define GIQL_FILL_ITEMS 16
#endif
constexpr int FILL_ITEMS_C2 = GIQL_FILL_ITEMS;  // pairs per thread of a fill block (tile = FILL_NT x this)

// grid cap of the gather-bound grid-stride kernels (take, mark, segment sum, checksum).  Unlike the
// streaming min/max and linearize passes (best at ONE resident wave of blocks), these were 2-5 %
// faster with 16384 blocks than with 2048.
#ifndef GIQL_STREAM_GRID
#define GIQL_STREAM_GRID 16384u
#endif

static inline u32 cdiv(u64 a, u64 b) { return (u32)((a + b - 1) / b); }
// a side's digit histogram replicas / the span pass's per-chromosome top-digit counts, as their owners zero them
constexpr size_t HIST_BYTES = (size_t)LIN_HIST_REPLICAS * 1024 * sizeof(u32);
constexpr size_t TOP_BYTES = (size_t)LIN_HIST_REPLICAS * MM_TOP_WORDS * sizeof(u32);

// ----------------------------------------------------------------- context
// The ping-pong buffers of one sort.  "Buffer 0" is where the rows are: run_sort_onesweep reads them there and leaves
// them there, whichever physical buffer its last pass wrote (flip()).
struct SortBufs {
  u32* key[2];
  u32* end[2];
  u32* rid[2];
  // which arrays travel with the keys (the kernels' MODE)
  SortPayload payload() const { return (SortPayload)((rid[0] ? 1 : 0) | (end[0] ? 2 : 0)); }
  // The ONLY exchange of the ping-pong pointers: a sort whose plan ends in physical buffer 1 makes that "buffer 0".
  // A copy or view of the buffers made before the sort does not follow: take one afterwards (keyed_by_end / follow).
  void flip() {
    std::swap(key[0], key[1]);
    std::swap(end[0], end[1]);
    std::swap(rid[0], rid[1]);
  }
  // the view that sorts by the end column, with the keys as its payload ...
  SortBufs keyed_by_end() const {
    SortBufs v = *this;
    std::swap(v.key, v.end);
    return v;
  }
  // ... and the owner catching up with what a sort did to that view (its flip included)
  void follow(const SortBufs& by_end) {
    for (int k = 0; k < 2; k++) {
      end[k] = by_end.key[k];
      key[k] = by_end.end[k];
      rid[k] = by_end.rid[k];
    }
  }
};

// Device pointers kept between inner_plan and inner_fill (all inside the arena).
struct InnerState {
  SortBufs sa, sb;   // sorted (key, end, rid) of A / B in buffer 0
  u32 nt1 = 0, nt2 = 0;
  int c1_items = C1_ITEMS_MAX;  // class-1 rows per thread of this plan (k_c1_count / k_c1_emit)
  u32* wlo1 = nullptr;   // class-1 S-window starts per block
  u64* c1_base = nullptr;  // class-1 output base per block
  // small B sides: class 1 takes the same count -> scan -> merge-path fill as class 2 (per-row arrays are
  // cheap there, and the fill stays coalesced when rows have many matches; k_c1_emit does not)
  bool c1_fill = false;
  u32 *lo1 = nullptr, *cnt1 = nullptr;
  u64* off1 = nullptr;
  u32* wlo2 = nullptr;
  u32* lo2 = nullptr;    // class-2 first matching B index per A row
  u32* cnt2 = nullptr;   // ... and the number of matches (kept for giql_hip_inner_plan_export_dev)
  u64* off2 = nullptr;   // class-2 exclusive output offsets
  // uniform-length form: 0 = general two-class join; 1 = B is uniform (queries =
  // A rows); 2 = A is uniform (queries = B rows)
  int uniform = 0;
};

// tuning constants the context does not vary
constexpr size_t C1_SMALL_ROWS = (size_t)4 << 20;  // class-1 sides up to this many rows take 2 rows per thread
// second stream: the smaller side's linearize + sort run beside the larger side's when that side is small enough to
// be latency-bound (a chain of ~10 short launches)
constexpr u64 OVERLAP_MAX_ROWS = (u64)4 << 20;

// The GIQL_HIP_* environment switches: read once by giql_hip_create (read_switches), constant afterwards.
struct Switches {
  bool classic_sort = false;  // GIQL_HIP_SORT=classic: three-launch radix passes
  int os_variant = 0;         // GIQL_HIP_OS_VARIANT: onesweep block shape (tuning)
  int os_order = 2;           // GIQL_HIP_OS_ORDER: the onesweep tile order a context starts with (see k_onesweep)
  u32 os_help_after = OS_HELP_AFTER;  // GIQL_HIP_OS_HELP_AFTER: look-back polls before a block helps
  int inject_timeout = 0;     // GIQL_HIP_INJECT_TIMEOUT=n (test hook): the n-th clean read-back reports a timeout
  bool no_uniform = false;    // GIQL_HIP_NO_UNIFORM=1: always run the general two-class join
  bool no_span_hist = false;  // GIQL_HIP_NO_SPAN_HIST=1: always linearize the fixed-length side (A/B aid)
  bool no_coarse_b = false;   // GIQL_HIP_NO_COARSE_B=1: the fixed-length B of SEMI / ANTI / COUNT is sorted on every digit
  double coarse_max_group_rows = 8.0;  // ... and coarsely only while the rows sharing their upper 24 key bits are at most this many on average
  bool no_fuse_count = false;  // GIQL_HIP_NO_FUSE_COUNT=1: the separate count kernel always
  // three-stage sort (two global passes on bits 16-31 + the in-LDS bucket sort, bucket_sort.hip.h) for sides of at
  // least local_min_rows rows whose 16-bit buckets hold between local_min_bucket_rows and local_max_bucket_rows rows
  // on average (smaller sides have too few rows per bucket to pay for a block each)
  bool no_local_sort = false;  // GIQL_HIP_NO_LOCAL_SORT=1: never
  u64 local_min_rows = 1u << 21;  // GIQL_HIP_LOCAL_MIN_ROWS (round 4: a floor only; the density bounds decide)
  double local_min_bucket_rows = 300.0;   // GIQL_HIP_LOCAL_MIN_BUCKET_ROWS (below: a block per bucket is mostly overhead)
  double local_max_bucket_rows = 2800.0;  // GIQL_HIP_LOCAL_MAX_BUCKET_ROWS
  // denser tables keep the form with NARROWER buckets (15 / 14 / 13 key bits, three global passes): sort_local_bits()
  bool no_narrow = false;  // GIQL_HIP_NO_NARROW_BUCKETS=1: 16 bits or nothing (round 3)
  int force_bits = 0;      // GIQL_HIP_LOCAL_BITS=w: every three-stage sort takes w (tests)
};

// What one call leaves for the next to speculate on, and the fallbacks a context keeps for good once taken.  Written
// by the calls that validate them (at their read-back); never reset.  A guess that missed makes its call return
// GIQL_STATUS_GUESS_MISSED with the guess dropped, and with_order_fallback repeats the call.
struct Guesses {
  bool local_sort = true;     // the three-stage sort; off for good once a bucket outgrew the LDS stage (GIQL_HIP_NO_LOCAL_SORT)
  int os_order = 2;           // onesweep tile order in force; 0 for good after a look-back timeout (GIQL_HIP_OS_ORDER)
  int inject_timeout = 0;     // clean read-backs left before the injected timeout (GIQL_HIP_INJECT_TIMEOUT)
  u64 last_span = 0;          // linearised span of the context's last call: the density guess of row_skip() / sort_is_local()
  bool last_no_irr = false;   // the previous plan met no irregular row
  bool nearest_two_sorts = false;  // NEAREST / group_rows: a B table with long equal-start runs was seen
  // NEAREST k = 1: both sides sorted straight from their raw columns (digits counted in the span pass, aligned layout;
  // no linearize pass) -- -1: not known yet (the next call probes the layout), 0: this data does not take the aligned
  // layout, 1: the previous call did
  int nearest_aligned = -1;
  bool spec_valid = false;    // INNER: the previous plan's form decision
  int spec_form = 0;
  i64 spec_len = 0;
  bool spec_aligned = false;  // ... and whether the aligned layout (histogram in the span pass) held
  bool spec_fuse_len_ok = false;  // the previous plan's query rows were all short enough for the fused windows
  // sorted inputs: a side the span pass found in (chrom id, start) order is not sorted again (plan labels, after the
  // exchange of sides)
  bool spec_sorted[2] = {false, false};
  // per-row operators (SEMI / ANTI / COUNT): the fixed length of B seen by the previous call (0 = B was not
  // fixed-length), speculated on like the INNER form
  bool row_spec_valid = false;
  i64 row_spec_len = 0;
  int spec_misses = 0;        // INNER plans repeated after a guess missed
  int local_resorts = 0;      // calls repeated with the four-pass sort
  int order_fallbacks = 0;    // calls repeated in the ticket order after a timeout
};

// Everything that lives for one call: reset by value in reset_stats() at the start of every call that reports
// stats (and so of every attempt with_order_fallback repeats).  The values giql_hip_get_stats reports stay until
// the next such call.
struct CallState {
  ZeroLedger zeroed;            // the bytes of the workspace this attempt zeroed in ONE memset up front (zero_ledger.h)
  // a sort's FIRST pass may rank its rows with LDS atomics (unstable: rows of equal digits in any order) when the caller
  // does not need equal keys in input order -- the INNER join's sides (onesweep.hip.h)
  bool first_unstable = false;
  int force_local = 0;          // +1 while a table index is built: the three-stage sort whatever the guesses say; -1: global passes only
  int index_bits = 16;          // the width of the index being built (force_local > 0)
  bool used_sorted[2] = {false, false};  // the call skipped that side's sort
  bool last_sort_local = false;  // the call sorted at least one side in three stages
  int last_local_bits = 16;      // ... the key bits of its buckets (the last bucket stage launched)
  // fused range count (fixed-length INNER form whose sorted side takes the three-stage sort): the bucket sort answers
  // the queries' bounds from LDS, the sorted keys never return to HBM (bucket_sort.hip.h)
  bool count_fused = false;
  // the join itself in the bucket stage (bucket_sort.hip.h, FUSE == 2): one-call form only, on the same guesses as the
  // early fill; the pairs leave from the bucket blocks, no sorted id / bound / offset array is written
  bool bucket_join = false;
};

// Which plan the context keeps between two calls: at most one, so one tag.  A plan is pointers into the workspace and
// is only as good as the record of who has touched that workspace since; the record is kept in three places and no
// operator writes it.  A plan entry point sets its tag as its last step (also on its way out with an empty result);
// begin_call drops whatever is kept, at the start of every call that resets the call state; claim_arena and
// ensure_arena drop it where the workspace is carved or replaced without a begin_call (giql_hip_reserve,
// giql_hip_chrom_spans_dev).  The fill and export entry points only test it.  (giql_hip_inner alone drops it once
// more, on return: its plans read columns staged for that call.)
enum class Plan { NONE, INNER, DISJOIN, CONTAINS };

// What inner_plan keeps for inner_fill / export (all inside the arena); written by inner_plan_core and by
// giql_hip_window_plan_dev.  Live while ctx->kept == Plan::INNER.
struct InnerPlan {
  bool plan_is_join = false;  // the pairs left from the bucket stage: no plan arrays (fill / export need a plan of their own)
  bool swapped = false;       // planned with the sides exchanged (giql_hip_inner_plan_dev_impl)
  // one-call join (giql_hip_inner_join_dev): the caller's outputs offered to the plan for a fill launched before the
  // host has learned the pair count (set around the plan), and whether that fill stood
  int32_t* fuse_a = nullptr;
  int32_t* fuse_b = nullptr;
  u64 fuse_cap = 0;
  bool fuse_done = false;
  giql_side side_a, side_b;
  u32 n_a = 0, n_b = 0;
  int n_chrom = 0;
  u64 n_reg = 0, n_irr = 0, n_c1 = 0;
  InnerState inner;
  u32* irr_a_list = nullptr;
  u32* irr_b_list = nullptr;
  u64* irr_off = nullptr;
  i64 widen = -1;  // >= 0: a within-distance plan (giql_hip_window_plan_dev); its irregular pairs follow the widened predicate
};

// What disjoin_plan keeps for disjoin_fill (all inside the arena).  Live while ctx->kept == Plan::DISJOIN.
struct DisjoinPlan {
  giql_side target;
  u64 total = 0;
  i64* chrom_base = nullptr;
  u64* off = nullptr;        // exclusive output offsets per target row
  u32* lo_first = nullptr;   // first breakpoint past the row's start | DJ_FIRST
  u32* bp = nullptr;         // distinct breakpoints
  u64* n_bp = nullptr;
  u32* ncov = nullptr;       // covered breakpoints below each (NULL in self mode)
  u32* cbp = nullptr;        // indices of the covered breakpoints
};

// What contain_plan keeps for contain_fill (the per-row arrays inside the arena, the per-tile ones in ct_buf).  Live
// while ctx->kept == Plan::CONTAINS.
struct ContainPlan {
  giql_side outer, inner;
  u32 n_o = 0, n_i = 0;
  int form = 0;              // 0 general (candidate tiles), 1 uniform inner side (exact range + k_fill)
  u64 n_cand = 0;            // T: candidates of the regular rows (general form)
  u64 n_reg = 0, n_irr = 0;  // pairs of regular rows / pairs involving an irregular row
  u32 n_tiles = 0;
  SortBufs so, si;           // sorted (key, end, rid) of the outer / inner side in buffer 0
  u32* lo = nullptr;         // first candidate per sorted outer row
  u64* coff = nullptr;       // exclusive offsets of the rows' candidate counts (uniform form: of their pairs)
  u32* ct_part = nullptr;    // first outer row per candidate tile
  u64* tile_off = nullptr;   // exclusive pair offsets per candidate tile
  u32* irr_o_list = nullptr;
  u32* irr_i_list = nullptr;
  u64* irr_off = nullptr;
};

struct giql_hip_ctx {
  explicit giql_hip_ctx(const Switches& s) : sw(s) {
    guess.local_sort = !s.no_local_sort;
    guess.os_order = s.os_order;
    guess.inject_timeout = s.inject_timeout;
  }
  const Switches sw;
  Guesses guess;
  CallState call;
  Plan kept = Plan::NONE;     // which of the three below is live
  InnerPlan plan;
  DisjoinPlan dj;
  ContainPlan ct;

  // device resources
  int device = 0;
  int n_cu = 256;             // compute units of the device
  DevArray<char> arena;       // the workspace (grown on demand; its bytes() are stats.workspace_bytes)
  DevArray<DevMeta> d_meta;
  DevMeta* h_meta = nullptr;  // pinned (released by giql_hip_destroy)
  DevArray<u32> part;         // fill partition (grown on demand)
  DevBuf stage_out;           // device staging of the host-buffer entry points' outputs (grown on demand)
  DevArray<char> xplan;       // scratch of giql_hip_fill_from_plan_dev (offsets + scan partials), grown on demand
  DevArray<char> ct_buf;      // per-tile arrays of a CONTAINS plan (sized by its candidate total), grown on demand
  DevArray<u64> d_scratch64;  // small device scratch (checksum)
  hipStream_t side_stream = nullptr;  // the second stream (SideChain)
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  DevArray<u32> bucket_qwin;  // [2 * BS_MAX_BUCKETS] query window per bucket
  DevArray<u32> bucket_bnd;   // [BS_MAX_BUCKETS + 1] bucket boundaries of the sort in flight
  DevArray<u32> bucket_big;   // [1 + BS_MAX_BUCKETS] buckets too large for LDS, queued for k_bucket_sort_big ([0] = count)

  // profiling
  int profiling = 0;          // 0 off, 1 every phase, 2 only profile_phase (the dominant kernel's)
  int profile_phase = GIQL_PH_SORT_SCATTER;
  std::vector<hipEvent_t> ev_pool;
  struct Span {
    int phase;
    hipEvent_t a, b;
  };
  std::vector<Span> spans;
  size_t ev_used = 0;
  giql_hip_stats stats;
};

// What the sort decisions (sort_plan.h) read of the context, in one place.  The header restates four constants of
// the kernel headers; they are the kernels' own.
static_assert(SORT_OS_BINS == OS_BINS && SORT_OS_MIN_TILE == OS_MIN_TILE && SORT_MIN_WBITS == BS_MIN_WBITS &&
              SORT_OS_DEFAULT_TILE == 1024 * 8, "sort_plan.h restates the kernel headers' constants");
static inline SortTuning sort_tuning(const giql_hip_ctx* ctx) {
  const Switches& sw = ctx->sw;
  SortTuning t;
  t.os_variant = sw.os_variant, t.local_min_rows = sw.local_min_rows, t.force_bits = sw.force_bits;
  t.local_min_bucket_rows = sw.local_min_bucket_rows, t.local_max_bucket_rows = sw.local_max_bucket_rows;
  t.no_narrow = sw.no_narrow, t.no_coarse_b = sw.no_coarse_b, t.coarse_max_group_rows = sw.coarse_max_group_rows;
  t.local_sort = ctx->guess.local_sort, t.last_span = ctx->guess.last_span;
  t.force_local = ctx->call.force_local, t.index_bits = ctx->call.index_bits, t.first_unstable = ctx->call.first_unstable;
  t.bucket_buffers = ctx->bucket_bnd.get() != nullptr;
  return t;
}

static int ensure_arena(giql_hip_ctx* ctx, size_t bytes, hipStream_t stream) {
  if (bytes <= ctx->arena.bytes()) return GIQL_OK;
  ctx->kept = Plan::NONE;  // (giql_hip_reserve: a new arena holds no plan)
  const size_t want = align_up(bytes + bytes / 8, (size_t)1 << 20);
  GIQL_TRY(ctx->arena.grow(bytes, want, stream, "the workspace"));
  if (getenv("GIQL_HIP_DEBUG_ADDR")) fprintf(stderr, "[giql_hip] arena %p + %zu bytes\n", ctx->arena.get(), want);
  return GIQL_OK;
}

// the fill's merge-path partition: at least `words` entries
static int grow_part(giql_hip_ctx* ctx, size_t words, hipStream_t stream) {
  return ctx->part.grow(words * sizeof(u32), (words + words / 4) * sizeof(u32), stream, "the fill partition");
}

// The workspace of a call: `carve` lays its buffers out from a base (nullptr: a dry run that returns the size), once
// to size the arena and once for real.  The call reuses what a plan keeps there: the plan is dropped, before the dry
// run (the INNER plan's carve writes the plan's own pointers).
template <typename Carve>
static int claim_arena(giql_hip_ctx* ctx, hipStream_t stream, Carve&& carve) {
  ctx->kept = Plan::NONE;
  GIQL_TRY(ensure_arena(ctx, carve(nullptr), stream));
  carve(ctx->arena);
  return GIQL_OK;
}

// ---------------------------------------------------------------- profiling
struct Phase {
  giql_hip_ctx* ctx;
  hipStream_t stream;
  int phase;
  hipEvent_t a = nullptr, b = nullptr;
  Phase(giql_hip_ctx* c, hipStream_t s, int ph, int launches = 1) : ctx(c), stream(s), phase(ph) {
    ctx->stats.phase_launches[ph] += launches;
    if (!ctx->profiling || (ctx->profiling == 2 && ph != ctx->profile_phase)) return;
    while (ctx->ev_used + 2 > ctx->ev_pool.size()) {
      hipEvent_t e;
      if (hipEventCreate(&e) != hipSuccess) return;
      ctx->ev_pool.push_back(e);
    }
    a = ctx->ev_pool[ctx->ev_used++];
    b = ctx->ev_pool[ctx->ev_used++];
    (void)hipEventRecord(a, stream);
  }
  ~Phase() {
    if (!a) return;
    (void)hipEventRecord(b, stream);
    ctx->spans.push_back({phase, a, b});
  }
};

// The one place that resets per-call state (at the start of every call that reports stats).
static void reset_stats(giql_hip_ctx* ctx) {
  memset(&ctx->stats, 0, sizeof(ctx->stats));
  ctx->call = CallState{};
  ctx->spans.clear();
  ctx->ev_used = 0;
}

// The start of every call that resets the call state, and the one rule of a plan's lifetime: the plan the context
// keeps is dropped here, whatever the call goes on to do -- also when it returns at once because a side is empty.
// (A check that fails before this point leaves the context as it was.)  n_a / n_b: the sizes the call reports.
static int begin_call(giql_hip_ctx* ctx, int64_t n_a = 0, int64_t n_b = 0, bool keep_join_plan = false) {
  HIP_TRY(hipSetDevice(ctx->device));
  if (!keep_join_plan || ctx->kept == Plan::CONTAINS) ctx->kept = Plan::NONE;
  reset_stats(ctx);
  ctx->stats.n_a = n_a;
  ctx->stats.n_b = n_b;
  return GIQL_OK;
}

// begin_call for the five calls that touch no workspace and are made while a plan is still wanted --
//   giql_hip_distance_dev   the within-distance join fills its plan, then asks for the pairs' distances;
//   giql_hip_take_dev, giql_hip_take_utf8_fill_dev, giql_hip_mark_dev, giql_hip_segment_sum_dev
//                           projections and reductions over row ids the caller holds, run between a plan and its fill.
// They keep an INNER or DISJOIN plan.  A CONTAINS plan goes all the same: its per-tile arrays (ct_buf) and the
// statistics its fill adds to belong to the call that made it.
static int begin_call_beside_plan(giql_hip_ctx* ctx, int64_t n_a = 0, int64_t n_b = 0) {
  return begin_call(ctx, n_a, n_b, true);
}

// The prologue of the operators on two sides: the checks, then begin_call with the sides' sizes.
static int check_side(const giql_side* s, const char* name);
static int begin_pair_call(giql_hip_ctx* ctx, const giql_side* a, const giql_side* b, int32_t n_chrom) {
  GIQL_TRY(check_side(a, "a"));
  GIQL_TRY(check_side(b, "b"));
  if (n_chrom < 0) return set_err(GIQL_ERR_INVALID, "n_chrom < 0");
  return begin_call(ctx, a->n, b->n);
}

// the onesweep sort's status words count rows in 30 bits
static int check_rows_fit(size_t na, size_t nb) {
  if (na > OS_MAX_ROWS || nb > OS_MAX_ROWS) return set_err(GIQL_ERR_INVALID, "side larger than 2^30 rows");
  return GIQL_OK;
}

// The frame of a call that zeroes workspace up front (zero_span): when it ends nothing is known to be zero any more,
// and the sort helpers zero their own histograms and status words again.
struct ZeroedScope {
  giql_hip_ctx* c;
  ~ZeroedScope() { c->call.zeroed.reset(); }
};

// What a helper does with a buffer that has to start at zero: skip the memset where the ledger hands the buffer over.
static int take_zeroed(giql_hip_ctx* ctx, hipStream_t st, void* p, size_t bytes) {
  if (!ctx->call.zeroed.take(p, bytes)) HIP_TRY(hipMemsetAsync(p, 0, bytes, st));
  return GIQL_OK;
}

// The one place that zeroes workspace up front: the memset, then the ledger's record of it.
static int zero_span(giql_hip_ctx* ctx, hipStream_t st, ZeroSpan s) {
  if (s.end <= s.off) return GIQL_OK;
  HIP_TRY(hipMemsetAsync(ctx->arena + s.off, 0, s.end - s.off, st));
  ctx->call.zeroed.add(ctx->arena + s.off, s.end - s.off);
  return GIQL_OK;
}

// A sort's first pass may rank by LDS atomics for a scope (CallState::first_unstable).
struct UnstableFirstPass {
  giql_hip_ctx* c;
  explicit UnstableFirstPass(giql_hip_ctx* ctx) : c(ctx) { c->call.first_unstable = true; }
  ~UnstableFirstPass() { c->call.first_unstable = false; }
};

// The three-stage sort forced on (+1: an index build) or off (-1: an indexed join's query side) for a scope.
struct ForceLocal {
  giql_hip_ctx* c;
  ForceLocal(giql_hip_ctx* ctx, int v) : c(ctx) { c->call.force_local = v; }
  ~ForceLocal() {
    c->call.force_local = 0;
    c->call.index_bits = 16;
  }
};

// Call only after the stream has been synchronised.
static void collect_spans(giql_hip_ctx* ctx) {
  if (!ctx->profiling) return;
  for (auto& s : ctx->spans) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) ctx->stats.phase_ms[s.phase] += ms;
  }
  ctx->spans.clear();
  ctx->ev_used = 0;
  float t = 0.f;
  for (int i = 0; i < GIQL_PH_N; i++) t += ctx->stats.phase_ms[i];
  ctx->stats.total_ms = t;
  ctx->stats.profiled = 1;
}

// The axis the last read-back saw: reported, and the density the next call's sort form follows.
static void note_span(giql_hip_ctx* ctx) {
  ctx->stats.span = (int64_t)ctx->h_meta->total_span;
  ctx->guess.last_span = ctx->h_meta->total_span;
}

// ------------------------------------------------------------ small helpers
static int check_side(const giql_side* s, const char* name) {
  if (!s) return set_err(GIQL_ERR_INVALID, "side %s is NULL", name);
  if (s->n < 0 || s->n > 0x7FFFFFF0ll)
    return set_err(GIQL_ERR_INVALID, "side %s: n=%lld outside [0, 2^31-16]", name, (long long)s->n);
  if (s->n > 0 && (!s->chrom || !s->start || !s->end))
    return set_err(GIQL_ERR_INVALID, "side %s: NULL column buffer", name);
  if (s->start_off < -1 || s->start_off > 0 || s->end_off < -1 || s->end_off > 1)
    return set_err(GIQL_ERR_INVALID, "side %s: canonical offsets (%d,%d) outside {0,-1}x{+1,0,-1}",
                   name, s->start_off, s->end_off);
  return GIQL_OK;
}

static SideView view_of(const giql_side& s) {
  SideView v;
  v.chrom = s.chrom;
  v.start = s.start;
  v.end = s.end;
  v.n = (u32)s.n;
  v.start_off = s.start_off;
  v.end_off = s.end_off;
  return v;
}

static int post_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    return set_err(GIQL_ERR_HIP, "kernel launch failed in %s: %s", what, hipGetErrorString(e));
  return GIQL_OK;
}

// exclusive scan of u32 counts; TOut in {u32,u64}; in-place allowed for u32.
// total_out2: a second place for the total (DevMeta::n_out ...), written by the spine kernel itself.
template <typename TOut>
static int run_scan(giql_hip_ctx* ctx, hipStream_t st, int phase, const u32* in, u64 n, TOut* out,
                    u64* bsums, u64* total_out, u64* total_out2 = nullptr) {
  if (n == 0) {
    if (total_out) HIP_TRY(hipMemsetAsync(total_out, 0, sizeof(u64), st));
    if (total_out2) HIP_TRY(hipMemsetAsync(total_out2, 0, sizeof(u64), st));
    return GIQL_OK;
  }
  const u32 nb = cdiv(n, SCAN_TILE);
  Phase ph(ctx, st, phase, 3);
  hipLaunchKernelGGL(k_scan_reduce, dim3(nb), dim3(SCAN_NT), 0, st, in, n, bsums);
  hipLaunchKernelGGL(k_scan_spine, dim3(1), dim3(1024), 0, st, bsums, nb, total_out, total_out2);
  hipLaunchKernelGGL((k_scan_down<TOut>), dim3(nb), dim3(SCAN_NT), 0, st, in, n, bsums, out);
  return post_launch("scan");
}

// The scan of 0/1 flags with the compaction in its down-sweep (SEMI / ANTI): the ids of the set flags, ascending, into
// rows_out; their number into DevMeta::n_out.  `spine_out`: where the spine leaves its exclusive block offsets.
static int run_scan_compact(giql_hip_ctx* ctx, hipStream_t st, const u32* flag, size_t n, u64* bsums, u64* spine_out,
                            int32_t* rows_out, const char* what) {
  const u32 nbk = cdiv(n, SCAN_TILE);
  Phase ph(ctx, st, GIQL_PH_SCAN, 3);
  hipLaunchKernelGGL(k_scan_reduce, dim3(nbk), dim3(SCAN_NT), 0, st, flag, (u64)n, bsums);
  hipLaunchKernelGGL(k_scan_spine, dim3(1), dim3(1024), 0, st, bsums, nbk, spine_out, &ctx->d_meta->n_out);
  hipLaunchKernelGGL(k_scan_down_compact, dim3(nbk), dim3(SCAN_NT), 0, st, flag, (u64)n, bsums, rows_out);
  return post_launch(what);
}

// The same over counts given as two bounds per row (cnt = hi - lo below the regular prefix, 0 past it):
// what the fused range count leaves.  The down-sweep rewrites `hi` as the counts.
static int run_scan_diff(giql_hip_ctx* ctx, hipStream_t st, int phase, u32* hi, u32* lo, u64 n, const u32* n_irr,
                         u64* out, u64* bsums, u64* total_out, u64* total_out2) {
  const u32 nb = cdiv(n, SCAN_TILE);
  Phase ph(ctx, st, phase, 3);
  hipLaunchKernelGGL(k_scan_reduce_diff, dim3(nb), dim3(SCAN_NT), 0, st, hi, lo, n, n_irr, bsums);
  hipLaunchKernelGGL(k_scan_spine, dim3(1), dim3(1024), 0, st, bsums, nb, total_out, total_out2);
  hipLaunchKernelGGL(k_scan_down_diff, dim3(nb), dim3(SCAN_NT), 0, st, hi, lo, n, n_irr, bsums, out);
  return post_launch("scan (bounds)");
}

// One launch: chained scan of the same bounds (status + ticket zeroed by the caller's previous kernel); out[n] =
// total, also to total_out2; part (optional): the fill's merge-path partition for tiles of 2^tile_log2 outputs.
static int run_scan_chain(giql_hip_ctx* ctx, hipStream_t st, int phase, const u32* hi, const u32* lo, u64 n,
                          const u32* n_irr, u64* out, u64* chain_status, u64* total_out2, u32* part, u32 tile_log2,
                          u32 part_cap) {
  const u32 nb = cdiv(n, SC_TILE);
  Phase ph(ctx, st, phase, 1);
  hipLaunchKernelGGL(k_scan_chain_diff, dim3(nb), dim3(SC_NT), 0, st, hi, lo, (u32)n, n_irr, chain_status,
                     reinterpret_cast<u32*>(chain_status + nb + 1), out, total_out2, part, tile_log2, part_cap);
  return post_launch("scan (chained)");
}

// Spans + linearised keys for both sides.
struct LinBufs {
  int* gmin;
  int* gmax;
  i64* chrom_base;
  u32* chrom_first;
  int* len_part;  // [2 sides][MM_MAX_BLOCKS][min,max]
  // histogram-in-the-span-pass form (INNER plan only; NULL elsewhere)
  u32* abase = nullptr;        // [MM_HIST_CHROMS] 2^24-aligned chromosome bases
  u32* top_partial = nullptr;  // [LIN_HIST_REPLICAS][MM_HIST_CHROMS][256]
  // the OTHER side's (the query side of the fixed-length form, when it is sorted from its raw columns too)
  u32* top_partial2 = nullptr;
  u32* hist_partial2 = nullptr;
};


// The range of the two sides' canonical offsets, widened by `pad`: the positions every chromosome gets beyond its
// rows' range on either end (the within-distance forms: 1, for the clamped ends of their widened rows --
// distance_kernels.hip.h).  run_spans hands the two numbers to k_chrom_offsets and key_widened_side clamps to them:
// both take them from here.
static void window_pads(const giql_side& a, const giql_side& b, int pad, int& lo_pad, int& hi_pad) {
  lo_pad = hi_pad = a.start_off;
  const int offs[3] = {a.end_off, b.start_off, b.end_off};
  for (int k = 0; k < 3; k++) {
    if (offs[k] < lo_pad) lo_pad = offs[k];
    if (offs[k] > hi_pad) hi_pad = offs[k];
  }
  lo_pad -= pad;
  hi_pad += pad;
}

// hist_side = 0 / 1 (with hist_partial and lb.abase / lb.top_partial): that side's span pass
// also counts the digits of its aligned keys (k_chrom_minmax<true>) and the chromosome bases
// are laid out 2^24-aligned when they fit (meta->aligned_ok).
static int run_spans(giql_hip_ctx* ctx, hipStream_t st, const giql_side& a, const giql_side& b,
                     int n_chrom, const LinBufs& lb, int hist_side = -1, u32* hist_partial = nullptr, int pad = 0) {
  const bool hist = hist_side >= 0 && hist_partial && lb.abase && lb.top_partial &&
                    n_chrom <= MM_HIST_CHROMS && (hist_side ? b.n : a.n) > 0;
  // both sides count their digits (lb.hist_partial2 / top_partial2 for the other one: only where they were zeroed
  // up front, there is no memset for them here)
  const ZeroLedger& zeroed = ctx->call.zeroed;
  const bool hist2 = hist && lb.hist_partial2 && lb.top_partial2 && (hist_side ? a.n : b.n) > 0 &&
                     zeroed.covers(lb.hist_partial2, HIST_BYTES) && zeroed.covers(lb.top_partial2, TOP_BYTES);
  // (the span pass takes every histogram it counts into: a side that is linearized after all finds its own taken)
  if (hist) {
    GIQL_TRY(take_zeroed(ctx, st, hist_partial, HIST_BYTES));
    GIQL_TRY(take_zeroed(ctx, st, lb.top_partial, TOP_BYTES));
  }
  if (hist2) {
    GIQL_TRY(take_zeroed(ctx, st, lb.hist_partial2, HIST_BYTES));
    GIQL_TRY(take_zeroed(ctx, st, lb.top_partial2, TOP_BYTES));
  }
  Phase ph(ctx, st, GIQL_PH_SPAN, 4);
  hipLaunchKernelGGL(k_init_minmax, dim3(cdiv((u64)n_chrom + 1, 256)), dim3(256), 0, st, lb.gmin,
                     lb.gmax, n_chrom, ctx->d_meta);
  const size_t lds = n_chrom <= MM_LDS_CHROMS ? (size_t)n_chrom * 2 * sizeof(int) : 0;
  const giql_side* sides[2] = {&a, &b};
  int nblk[2] = {0, 0};
  if (a.n > 0 && b.n > 0) {
    // both sides in ONE launch: the grid (one resident wave of 512-thread blocks) is shared in proportion to the rows
    MmSide ms[2];
    const double tot = (double)a.n + (double)b.n;
    for (int k = 0; k < 2; k++) {
      const giql_side& s = *sides[k];
      const bool with_hist = hist && (k == hist_side || hist2);
      u32* const hp = k == hist_side ? hist_partial : lb.hist_partial2;
      u32 grid = (u32)((double)MM_MAX_BLOCKS * (double)s.n / tot + 0.5);
      const u32 need = cdiv((u64)s.n, (u64)MM_NT_HIST * 4);   // a block per tile at most
      if (grid > need) grid = need;
      if (grid < 1) grid = 1;
      nblk[k] = (int)grid;
      ms[k].chrom = s.chrom;
      ms[k].start = s.start;
      ms[k].end = s.end;
      ms[k].n = (i64)s.n;
      ms[k].len_bias = s.end_off - s.start_off;
      ms[k].start_off = with_hist ? s.start_off : 0;
      ms[k].hist = !with_hist ? 0 : span_hist_mode(sort_tuning(ctx), (size_t)s.n);  // which digits: as the side's sort will need them
      ms[k].nblk = grid;
      ms[k].hist_partial = with_hist ? hp : nullptr;
      ms[k].top_partial = with_hist ? (k == hist_side ? lb.top_partial : lb.top_partial2) : nullptr;
    }
    hipLaunchKernelGGL((k_chrom_minmax2<MM_NT_HIST>), dim3(ms[0].nblk + ms[1].nblk), dim3(MM_NT_HIST), lds, st, ms[0], ms[1],
                       n_chrom, lb.gmin, lb.gmax, ctx->d_meta, lb.len_part);
  } else
  for (int k = 0; k < 2; k++) {
    const giql_side& s = *sides[k];
    if (s.n == 0) continue;
    const bool with_hist = hist && (k == hist_side || hist2);
    u32* const hp = k == hist_side ? hist_partial : lb.hist_partial2;
    u32* const tp = k == hist_side ? lb.top_partial : lb.top_partial2;
    u32 grid = cdiv((u64)s.n, (u64)(with_hist ? MM_NT_HIST : MM_NT) * MM_ITEMS);
    if (grid > (u32)MM_MAX_BLOCKS) grid = MM_MAX_BLOCKS;
    nblk[k] = (int)grid;
    if (with_hist && span_hist_mode(sort_tuning(ctx), (size_t)s.n) == 2)  // the low digits are sorted in LDS: not counted
      hipLaunchKernelGGL((k_chrom_minmax<2, MM_NT_HIST>), dim3(grid), dim3(MM_NT_HIST), lds, st, s.chrom, s.start, s.end,
                         (i64)s.n, n_chrom, lb.gmin, lb.gmax, ctx->d_meta, s.end_off - s.start_off, k,
                         lb.len_part, s.start_off, hp, tp);
    else if (with_hist)
      hipLaunchKernelGGL((k_chrom_minmax<1, MM_NT_HIST>), dim3(grid), dim3(MM_NT_HIST), lds, st, s.chrom, s.start, s.end,
                         (i64)s.n, n_chrom, lb.gmin, lb.gmax, ctx->d_meta, s.end_off - s.start_off, k,
                         lb.len_part, s.start_off, hp, tp);
    else
      hipLaunchKernelGGL((k_chrom_minmax<0, MM_NT>), dim3(grid), dim3(MM_NT), lds, st, s.chrom, s.start, s.end,
                         (i64)s.n, n_chrom, lb.gmin, lb.gmax, ctx->d_meta, s.end_off - s.start_off, k,
                         lb.len_part, 0, (u32*)nullptr, (u32*)nullptr);
  }
  int omin, omax;
  window_pads(a, b, pad, omin, omax);
  hipLaunchKernelGGL(k_chrom_offsets, dim3(1), dim3(256), 0, st, lb.gmin, lb.gmax, n_chrom, omin,
                     omax, lb.chrom_base, lb.chrom_first, ctx->d_meta, lb.len_part, nblk[0], nblk[1],
                     hist ? 1 : 0, lb.abase);
  return post_launch("spans");
}

// A column's digit counts: the histogram replicas a pass counts into and the digit bases made of them (both or neither).
struct DigitCounts {
  u32* hist = nullptr;
  u32* base = nullptr;
};
// Scratch shared by the single-output operators: histogram replicas, digit bases,
// onesweep status words (+ tile-claim state) for one side at a time.
struct OsScratch {
  u32 *hist = nullptr, *gbase = nullptr, *hist_e = nullptr, *gbase_e = nullptr;
  u32* status = nullptr;
  DigitCounts starts() const { return {hist, gbase}; }
  DigitCounts ends() const { return {hist_e, gbase_e}; }
};

// One linearize pass: whose rows, where they go, and what else the pass does on the way.
enum class Side { A = 0, B = 1 };
struct LinTarget {
  u32* keys = nullptr;
  u32* ends = nullptr;      // NULL: the end keys are not wanted
  u32* irr_list = nullptr;
  static LinTarget keys_only(u32* keys, u32* irr_list) { return {keys, nullptr, irr_list}; }
  static LinTarget keys_ends(u32* keys, u32* ends, u32* irr_list) { return {keys, ends, irr_list}; }
};
struct LinOptions {
  bool keep_irregular = false;  // irregular rows keep their real key (they are not listed and given the sentinel)
  bool skip_end = false;        // a side known to hold no irregular row: its end column is not read
  DigitCounts starts, ends;     // also produce the onesweep digit offsets of the start keys / of the end keys
  LinOptions& keeping_irregular() { keep_irregular = true; return *this; }
  LinOptions& without_end_column(bool yes = true) { skip_end = yes; return *this; }
  LinOptions& counting_starts(DigitCounts d) { starts = d; return *this; }
  LinOptions& counting_ends(DigitCounts d) { ends = d; return *this; }
};

static int run_linearize(giql_hip_ctx* ctx, hipStream_t st, const giql_side& s, int n_chrom, const LinBufs& lb,
                         Side which, const LinTarget& out, const LinOptions& opt = LinOptions()) {
  if (s.n == 0) return GIQL_OK;
  const int* end_col = opt.skip_end ? (const int*)nullptr : s.end;
  u32* const hist_partial = opt.starts.hist;
  u32* const hist_end = opt.ends.hist;
  // (a plan zeroes its histograms once, up front -- but this one may hold the span pass's counts of a side that
  // turned out to need the linearize pass after all, layout or form guess not taken: the span pass took it then)
  if (hist_partial) GIQL_TRY(take_zeroed(ctx, st, hist_partial, HIST_BYTES));
  if (hist_end) GIQL_TRY(take_zeroed(ctx, st, hist_end, HIST_BYTES));
  Phase ph(ctx, st, GIQL_PH_LINEARIZE, hist_partial ? 2 : 1);
  u32 grid = cdiv((u64)s.n, LIN_NT);
  if (grid > (u32)LIN_MAX_BLOCKS) grid = LIN_MAX_BLOCKS;
  if (hist_end)
    hipLaunchKernelGGL((k_linearize<true>), dim3(grid), dim3(LIN_NT), 0, st, s.chrom, s.start, end_col,
                       (u32)s.n, s.start_off, s.end_off, n_chrom, lb.chrom_base, out.keys, out.ends, out.irr_list,
                       ctx->d_meta, (int)which, opt.keep_irregular ? 1 : 0, hist_partial, hist_end);
  else
    hipLaunchKernelGGL((k_linearize<false>), dim3(grid), dim3(LIN_NT), 0, st, s.chrom, s.start, end_col,
                       (u32)s.n, s.start_off, s.end_off, n_chrom, lb.chrom_base, out.keys, out.ends, out.irr_list,
                       ctx->d_meta, (int)which, opt.keep_irregular ? 1 : 0, hist_partial, (u32*)nullptr);
  if (hist_partial)
    hipLaunchKernelGGL(k_digit_offsets, dim3(4), dim3(256), 0, st, hist_partial,
                       (u32)LIN_HIST_REPLICAS, opt.starts.base);
  if (hist_end)
    hipLaunchKernelGGL(k_digit_offsets, dim3(4), dim3(256), 0, st, hist_end, (u32)LIN_HIST_REPLICAS,
                       opt.ends.base);
  return post_launch("linearize");
}

// ---------------------------------------------------------------------------------------------- the sort driver
// Onesweep LSD sort, one launch per global pass; input and result in buffer 0.  What a sort does -- how many passes,
// on which digits, between which buffers, the bucket stage that follows, the status words to zero, the bytes each
// phase reports -- is one SortPlan (sort_plan.h, plan_sort); run_sort_onesweep builds it, zeroes what it says and
// launches what it says.

// Calls f(std::integral_constant<int, M>{}) for the M among Ms that equals m: how a run-time payload, FUSE form or
// bucket width reaches a kernel's template arguments -- the one dispatcher of every kernel the driver launches.
// false: m is none of Ms and nothing was called (run_sort_onesweep refuses such a request before it launches anything).
template <int... Ms, typename F>
static inline bool dispatch_int(int m, F&& f) {
  return ((m == Ms && (f(std::integral_constant<int, Ms>{}), true)) || ...);
}

// fuse (three-stage (key, rid) sorts only): the bucket sort also answers the range bounds of the
// fixed-length INNER form's query rows and does not store the sorted keys (bucket_sort.hip.h).
struct FuseCount {
  BsFuse dev;
  u32 nq_total;
  const u32* irr_q;
  const u32* gbq3;      // the query sort's top-digit offsets
  u32 key_mask;         // 0xFFFFFF00 when the query side was sorted without its lowest digit
  const int* len_max_q; // DevMeta: longest regular query row
  u32* zero_ptr;        // words the bounds kernel zeroes on the way (the chained scan's status + ticket)
  u32 zero_words;
  bool join = false;    // FUSE == 2: the bucket blocks write the pairs themselves (dev.row_q / row_s / cap / cursor)
  bool general = false; // FUSE == 3: ... of the two-class join (rows of any length, (key, end, rid) sorts)
  const int* len_max_u = nullptr;  // DevMeta: longest row of the sorted side (general form: how far the windows reach up)
  SortFuse kind() const { return general ? SortFuse::GENERAL_JOIN : join ? SortFuse::JOIN : SortFuse::BOUNDS; }
};

// One sort of n rows in a SortBufs.  rows() names what every sort has; the rest is set by name.
struct SortRequest {
  u32 n = 0;
  const u32* digit_base = nullptr;  // [4][OS_BINS] exclusive digit offsets of the keys (k_digit_offsets)
  u32* status = nullptr;            // 4 * os_pass_words(n) words; the passes' share is zeroed here unless the call's one memset covered it
  bool keep_rids = false;           // the rid buffer already holds row ids (second sort of a two-key sort)
  // the first pass builds the keys from that side's raw (chrom, start) columns and the 2^24-aligned chromosome bases
  // instead of reading key[0] (k_onesweep<.., KEYGEN>; sorts with row ids, default block shape only)
  const giql_side* keygen = nullptr;
  const u32* abase = nullptr;
  // global-passes form only: that many low digits are left unsorted -- rows come out ordered by key >> 8 (>> 16).  For
  // QUERY sides whose order only serves locality (neighbouring rows search neighbouring ranges)
  int skip_digits = 0;
  const FuseCount* fuse = nullptr;  // the bucket stage also answers the other side's query rows
  bool presorted = false;           // the side arrives sorted: no scatter pass

  static SortRequest rows(u32 n, const u32* digit_base, u32* status) {
    SortRequest r;
    r.n = n, r.digit_base = digit_base, r.status = status;
    return r;
  }
  SortRequest& keeping_rids() { keep_rids = true; return *this; }
  SortRequest& keys_from(const giql_side* side, const u32* aligned_base) { keygen = side, abase = aligned_base; return *this; }
  SortRequest& skipping_digits(int k) { skip_digits = k; return *this; }
  SortRequest& fused_with(const FuseCount* f) { fuse = f; return *this; }
  SortRequest& already_sorted(bool yes) { presorted = yes; return *this; }
  SortOptions options() const {
    SortOptions o;
    o.keep_rids = keep_rids;
    o.keygen = keygen != nullptr;
    o.skip_digits = skip_digits;
    o.fuse = fuse ? fuse->kind() : SortFuse::NONE;
    o.fuse_queries = fuse ? fuse->nq_total : 0;
    o.presorted = presorted;
    return o;
  }
};
// the sorts of an operator's scratch: by the digit bases of its start keys / of its end keys, through its status words
static inline SortRequest sort_by_start(const OsScratch& os, size_t n) { return SortRequest::rows((u32)n, os.gbase, os.status); }
static inline SortRequest sort_by_end(const OsScratch& os, size_t n) { return SortRequest::rows((u32)n, os.gbase_e, os.status); }
static inline SortPlan plan_of(const giql_hip_ctx* ctx, const SortBufs& sb, const SortRequest& rq) {
  return plan_sort(sort_tuning(ctx), rq.n, sb.payload(), rq.options());
}

// one global pass that reads the keys (block shape NT x ITEMS)
template <int NT, int ITEMS>
static void launch_onesweep(giql_hip_ctx* ctx, hipStream_t st, const SortBufs& sb, const SortPass& p, u32 n,
                            const u32* gbase, u32* status, u32* claim) {
  const u32 grid = cdiv(n, NT * ITEMS);  // one block per tile
  const u32* rin = (p.first || !sb.rid[0]) ? (const u32*)nullptr : sb.rid[p.src];
  dispatch_int<0, 1, 2, 3>((int)sb.payload(), [&](auto mode) {
    hipLaunchKernelGGL((k_onesweep<decltype(mode)::value, NT, ITEMS>), dim3(grid), dim3(NT), 0, st, sb.key[p.src],
                       sb.end[0] ? sb.end[p.src] : (const u32*)nullptr, rin, sb.key[p.dst],
                       sb.end[0] ? sb.end[p.dst] : (u32*)nullptr, sb.rid[0] ? sb.rid[p.dst] : (u32*)nullptr, n,
                       p.digit * 8, gbase, status, claim, ctx->d_meta, ctx->guess.os_order, ctx->sw.os_help_after,
                       (const u32*)nullptr, 0u, 0u, p.unstable ? 1 : 0);
  });
}

// ... and the first pass that builds them from the raw columns
static void launch_onesweep_keygen(giql_hip_ctx* ctx, hipStream_t st, const SortBufs& sb, const SortPass& p, u32 n,
                                   const u32* gbase, u32* status, u32* claim, const giql_side& raw, const u32* abase) {
  const u32 grid = cdiv(n, 1024 * 8);
  const u32 *start = reinterpret_cast<const u32*>(raw.start), *chrom = reinterpret_cast<const u32*>(raw.chrom);
  // (key, rid): start, chrom.  (key, end, rid): start, end, chrom -- the end keys are built from the raw end column as well
  dispatch_int<1, 3>((int)sb.payload(), [&](auto mode) {
    constexpr bool ENDS = decltype(mode)::value == 3;
    hipLaunchKernelGGL((k_onesweep<decltype(mode)::value, 1024, 8, true>), dim3(grid), dim3(1024), 0, st, start,
                       ENDS ? reinterpret_cast<const u32*>(raw.end) : chrom, ENDS ? chrom : (const u32*)nullptr,
                       sb.key[p.dst], ENDS ? sb.end[p.dst] : (u32*)nullptr, sb.rid[p.dst], n, p.digit * 8, gbase, status, claim, ctx->d_meta,
                       ctx->guess.os_order, ctx->sw.os_help_after, abase, (u32)raw.start_off,
                       ENDS ? (u32)raw.end_off : 0u, p.unstable ? 1 : 0);
  });
}

// The global passes of a plan: one event pair around them (an event record between two launches costs the
// stream ~8 us of idle time; the per-launch time is phase time / launches).
static void launch_passes(giql_hip_ctx* ctx, hipStream_t st, const SortBufs& sb, const SortRequest& rq, const SortPlan& plan) {
  Phase ph(ctx, st, GIQL_PH_SORT_SCATTER, plan.n_pass);
  for (int k = 0; k < plan.n_pass; k++) {
    const SortPass& p = plan.pass[k];
    u32* stat = rq.status + k * plan.pass_stride;
    u32* claim = stat + plan.pass_stride - 16;  // the pass's ticket word
    const u32* gb = rq.digit_base + p.digit * OS_BINS;
    ctx->stats.phase_bytes[GIQL_PH_SORT_SCATTER] += p.bytes;
    if (p.keygen) {
      launch_onesweep_keygen(ctx, st, sb, p, rq.n, gb, stat, claim, *rq.keygen, rq.abase);
      continue;
    }
    switch (ctx->sw.os_variant) {  // block-shape sweep (tools/os_variants.py); default 1024 x 8
      case 1: launch_onesweep<512, 8>(ctx, st, sb, p, rq.n, gb, stat, claim); break;
      case 2: launch_onesweep<512, 16>(ctx, st, sb, p, rq.n, gb, stat, claim); break;
      case 3: launch_onesweep<256, 16>(ctx, st, sb, p, rq.n, gb, stat, claim); break;
      case 4: launch_onesweep<1024, 4>(ctx, st, sb, p, rq.n, gb, stat, claim); break;
      case 5: case 7: launch_onesweep<1024, 12>(ctx, st, sb, p, rq.n, gb, stat, claim); break;
      default: launch_onesweep<1024, 8>(ctx, st, sb, p, rq.n, gb, stat, claim); break;
    }
  }
}

// The presorted form: no scatter pass, one streaming pass for what a sort would have left in buffer 0.
static int launch_sorted_input(giql_hip_ctx* ctx, hipStream_t st, const SortBufs& sb, const SortRequest& rq, const SortPlan& plan) {
  Phase ph(ctx, st, GIQL_PH_SORT_SCATTER, 1);
  const u32 n = rq.n;
  u32 grid = cdiv(n, 256 * 8);
  if (grid > GIQL_STREAM_GRID) grid = GIQL_STREAM_GRID;
  ctx->stats.phase_bytes[GIQL_PH_SORT_SCATTER] += plan.stream_bytes;
  if (plan.stream == StreamKernel::KEYGEN)
    dispatch_int<0, 1, 2, 3>((int)sb.payload(), [&](auto mode) {
      hipLaunchKernelGGL(k_keygen_stream<decltype(mode)::value>, dim3(grid), dim3(256), 0, st, rq.keygen->chrom,
                         rq.keygen->start, rq.keygen->end, n, rq.abase, (u32)rq.keygen->start_off,
                         (u32)rq.keygen->end_off, sb.key[0], sb.end[0], sb.rid[0]);
    });
  else if (plan.stream == StreamKernel::IOTA)
    hipLaunchKernelGGL(k_iota, dim3(grid), dim3(256), 0, st, sb.rid[0], n);
  return post_launch("sorted input (no sort)");
}

// The bucket stage: the rows are in buffer 0, ordered by key >> wbits; bucket boundaries, then one block per bucket,
// then the queue of buckets too large for LDS (almost always an empty launch).
//   plain: the three launches are one phase (SORT_LOCAL); only the bucket width travels to the kernels;
//   fused (bounds only, FUSE 1; the whole join, FUSE 2 / 3): each launch a phase of its own so that the stage's ONE
//     heavy kernel can be timed alone -- the boundaries and query windows (COUNT), the bucket kernel (SORT_LOCAL), the
//     queue (AUX).  (key, rid) rows + the query side's bounds: the sorted keys never leave the CU.
static int launch_bucket_stage(giql_hip_ctx* ctx, hipStream_t st, const SortBufs& sb, const SortPlan& plan, u32 n,
                               const u32* digit_base, const FuseCount* fuse_count) {
  const bool fused = plan.stage == BucketStage::FUSED;
  const u32 wbits = (u32)plan.wbits;
  const u32 buckets = bs_n_buckets(wbits);
  const u32* gb3 = digit_base + 3 * OS_BINS;
  BsFuse dev;
  if (fused) dev = fuse_count->dev;
  dev.wbits = wbits;
  ctx->call.last_local_bits = plan.wbits;
  ctx->stats.phase_bytes[GIQL_PH_SORT_LOCAL] += plan.stage_bytes;
  auto sort_buckets = [&](auto payload, auto fuse) {
    dispatch_int<0, 1>(wbits == 16 ? 1 : 0, [&](auto w16) {
      hipLaunchKernelGGL((k_bucket_sort<decltype(payload)::value, decltype(fuse)::value, decltype(w16)::value != 0>),
                         dim3(buckets), dim3(BS_NT), 0, st, sb.key[0], sb.end[0], sb.rid[0], ctx->bucket_bnd, ctx->d_meta,
                         ctx->bucket_big, dev);
    });
  };
  auto sort_queue = [&](auto payload, auto fuse) {
    hipLaunchKernelGGL((k_bucket_sort_big<decltype(payload)::value, decltype(fuse)::value>), dim3(ctx->n_cu), dim3(BS_NT),
                       0, st, sb.key[0], sb.end[0], sb.rid[0], sb.key[1], sb.end[0] ? sb.end[1] : (u32*)nullptr,
                       sb.rid[0] ? sb.rid[1] : (u32*)nullptr, ctx->bucket_bnd, ctx->bucket_big, dev);
  };
  if (!fused) {
    HIP_TRY(hipMemsetAsync(ctx->bucket_big, 0, sizeof(u32), st));
    Phase ph(ctx, st, GIQL_PH_SORT_LOCAL, 3);
    hipLaunchKernelGGL(k_bucket_bounds, dim3(cdiv((u64)buckets + 1, 256)), dim3(256), 0, st, sb.key[0], n, gb3,
                       ctx->bucket_bnd, wbits);
    dispatch_int<0, 1, 2, 3>(plan.stage_payload, [&](auto payload) {
      sort_buckets(payload, std::integral_constant<int, 0>{});
      sort_queue(payload, std::integral_constant<int, 0>{});
    });
    return GIQL_OK;
  }
  const FuseCount& fc = *fuse_count;
  ctx->call.count_fused = true;
  ctx->call.bucket_join = fc.join;
  {
    Phase ph(ctx, st, GIQL_PH_COUNT, 1);
    hipLaunchKernelGGL(k_bucket_bounds_fused, dim3(cdiv((u64)3 * buckets + 1, 256)), dim3(256), 0, st, sb.key[0], n, gb3,
                       ctx->bucket_bnd, ctx->bucket_big, dev, fc.nq_total, fc.irr_q, fc.gbq3, fc.key_mask, fc.len_max_q,
                       fc.zero_ptr, fc.zero_words, fc.len_max_u);
  }
  // the payload a fused form reads follows from the form: (key, end, rid) for the general join, else (key, rid)
  auto with_form = [&](auto&& launch) {
    dispatch_int<1, 2, 3>(plan.stage_fuse, [&](auto fuse) {
      launch(std::integral_constant<int, decltype(fuse)::value == 3 ? 3 : 1>{}, fuse);
    });
  };
  {
    Phase ph(ctx, st, GIQL_PH_SORT_LOCAL, 1);
    with_form(sort_buckets);
  }
  Phase ph(ctx, st, GIQL_PH_AUX, 1);
  with_form(sort_queue);
  return GIQL_OK;
}

static int run_sort_onesweep(giql_hip_ctx* ctx, hipStream_t st, SortBufs& sb, const SortRequest& rq) {
  if (rq.n == 0) return GIQL_OK;
  const SortPlan plan = plan_of(ctx, sb, rq);
  if (rq.keygen && !plan.presorted && !has_rid(sb.payload()))
    return set_err(GIQL_ERR_STATE, "internal: a sort pass that builds its keys writes row ids, this sort carries none");
  if (plan.presorted) {
    GIQL_TRY(launch_sorted_input(ctx, st, sb, rq, plan));
    if (plan.stage == BucketStage::NONE) return GIQL_OK;
  } else {
    GIQL_TRY(take_zeroed(ctx, st, rq.status, plan.status_words * sizeof(u32)));
    launch_passes(ctx, st, sb, rq, plan);
    if (plan.result_buf) sb.flip();  // the rows are in physical buffer 1: make that "buffer 0"
  }
  if (plan.stage != BucketStage::NONE) {
    ctx->call.last_sort_local = true;
    GIQL_TRY(launch_bucket_stage(ctx, st, sb, plan, rq.n, rq.digit_base, rq.fuse));
  }
  return post_launch(plan.presorted                         ? "bucket stage (sorted input, fused count)"
                     : plan.stage == BucketStage::FUSED ? "onesweep sort (fused count)"
                                                        : "onesweep sort");
}

// The stable two-key sort: (key, end) lexicographic order = stable sort by end, then stable sort by key (which keeps the
// row ids the first sort left).  Both sorts go through the one set of status words; the digit bases are the scratch's
// two (starts: the keys, ends: the end keys).
// The FIRST sort runs on a view of the buffers with key and end exchanged.  run_sort_onesweep leaves its result in what
// it then CALLS buffer 0 -- after an odd number of passes (three: a query side sorted without its lowest digit, a side
// with buckets narrower than 2^16 keys) that is the other physical buffer, and SortBufs::flip() says so on the view.
// The owner of the buffers has to follow (SortBufs::follow), or its second sort starts from the unsorted copy (round 4:
// found by the soak on a context forced to 8,192-key buckets -- ties among equal starts came out in input order).
static int run_sort_two_keys(giql_hip_ctx* ctx, hipStream_t st, SortBufs& sb, u32 n, const OsScratch& os) {
  SortBufs by_end = sb.keyed_by_end();
  GIQL_TRY(run_sort_onesweep(ctx, st, by_end, sort_by_end(os, n)));
  sb.follow(by_end);
  return run_sort_onesweep(ctx, st, sb, sort_by_start(os, n).keeping_rids());
}

// Stable LSD radix sort; input in buffer 0, result in buffer 0 (4 passes).
// rids: identity on the first pass.  Payload-less when bufs.end[0] == nullptr; (key, payload) rows without row ids
// when only bufs.rid[0] is.
// passes (0..4): keys below 2^(8 * passes) need no pass on their upper digits; after an odd number the result lies in
// the other physical buffer, which then becomes "buffer 0" (SortBufs::flip).
static int run_sort(giql_hip_ctx* ctx, hipStream_t st, SortBufs& sb, u32 n, u32* tile_hist,
                    u64* bsums, int passes = 4) {
  if (n == 0 || passes == 0) return GIQL_OK;
  const u32 n_tiles = cdiv(n, RS_TILE);
  for (int pass = 0; pass < passes; pass++) {
    const int src = pass & 1, dst = src ^ 1;
    const int shift = pass * 8;
    {
      Phase ph(ctx, st, GIQL_PH_SORT_HIST);
      hipLaunchKernelGGL(k_radix_hist, dim3(n_tiles), dim3(RS_NT), 0, st, sb.key[src], n, shift,
                         n_tiles, tile_hist);
    }
    GIQL_TRY(run_scan<u32>(ctx, st, GIQL_PH_SORT_SCAN, tile_hist, (u64)n_tiles * RS_BINS, tile_hist,
                           bsums, nullptr));
    {
      Phase ph(ctx, st, GIQL_PH_SORT_SCATTER);
      if (sb.end[0] && !sb.rid[0]) {  // (key, payload) rows without row ids
        hipLaunchKernelGGL((k_radix_scatter<true, false>), dim3(n_tiles), dim3(RS_NT), 0, st, sb.key[src],
                           sb.end[src], (const u32*)nullptr, sb.key[dst], sb.end[dst], (u32*)nullptr, n, shift,
                           n_tiles, tile_hist);
      } else if (sb.end[0]) {
        hipLaunchKernelGGL((k_radix_scatter<true>), dim3(n_tiles), dim3(RS_NT), 0, st, sb.key[src],
                           sb.end[src], pass == 0 ? (const u32*)nullptr : sb.rid[src], sb.key[dst],
                           sb.end[dst], sb.rid[dst], n, shift, n_tiles, tile_hist);
      } else {
        hipLaunchKernelGGL((k_radix_scatter<false>), dim3(n_tiles), dim3(RS_NT), 0, st, sb.key[src],
                           (const u32*)nullptr, (const u32*)nullptr, sb.key[dst], (u32*)nullptr,
                           (u32*)nullptr, n, shift, n_tiles, tile_hist);
      }
    }
  }
  if (passes & 1) sb.flip();
  return post_launch("radix sort");
}

static int run_pmax(giql_hip_ctx* ctx, hipStream_t st, const u32* in, u32 n, u32* out, u32* bmax) {
  if (n == 0) return GIQL_OK;
  const u32 nb = cdiv(n, PM_TILE);
  Phase ph(ctx, st, GIQL_PH_AUX, 3);
  hipLaunchKernelGGL(k_pmax_reduce, dim3(nb), dim3(PM_NT), 0, st, in, n, bmax);
  hipLaunchKernelGGL(k_pmax_spine, dim3(1), dim3(1024), 0, st, bmax, nb);
  hipLaunchKernelGGL(k_pmax_down, dim3(nb), dim3(PM_NT), 0, st, in, n, bmax, out);
  return post_launch("prefix max");
}

static int read_meta(giql_hip_ctx* ctx, hipStream_t st) {
  HIP_TRY(hipMemcpyAsync(ctx->h_meta, ctx->d_meta, sizeof(DevMeta), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  int status = ctx->h_meta->status;
  // test hook (GIQL_HIP_INJECT_TIMEOUT=n): the n-th clean read-back of the context reports a timeout
  if (ctx->guess.inject_timeout > 0 && ctx->guess.os_order != 0 && status == 0 && --ctx->guess.inject_timeout == 0)
    status = ctx->h_meta->status = GIQL_ERR_HIP;
  if (status == GIQL_STATUS_RESORT)  // internal: with_order_fallback repeats the call with the four-pass sort
    return set_err(GIQL_STATUS_RESORT, "a 16-bit key bucket holds more than %u rows", BS_CAP);
  if (status == GIQL_ERR_HIP)
    return set_err(GIQL_ERR_HIP, "onesweep look-back timed out (tile order %d)", ctx->guess.os_order);
  if (status == GIQL_ERR_CHROM)
    return set_err(GIQL_ERR_CHROM, "a chrom id is outside [0, n_chrom)");
  if (status == GIQL_ERR_SPAN)
    return set_err(GIQL_ERR_SPAN,
                   "linearised coordinate span %llu does not fit 32 bits; shard the chromosomes "
                   "into groups (giql_amd.shard) and join each group",
                   (unsigned long long)ctx->h_meta->total_span);
  if (status != 0) return set_err(status, "device reported status %d", status);
  return GIQL_OK;
}

static void common_sizes(Carver& c, int n_chrom, LinBufs& lb) {
  lb.gmin = c.take<int>((size_t)n_chrom);
  lb.gmax = c.take<int>((size_t)n_chrom);
  lb.chrom_base = c.take<i64>((size_t)n_chrom);
  lb.chrom_first = c.take<u32>((size_t)n_chrom + 1);
  lb.len_part = c.take<int>((size_t)2 * MM_MAX_BLOCKS * 2);
}

static void sort_sizes(Carver& c, size_t n, SortBufs& sb, bool end, bool rid) {
  for (int k = 0; k < 2; k++) {
    sb.key[k] = c.take<u32>(n);
    sb.end[k] = end ? c.take<u32>(n) : nullptr;
    sb.rid[k] = rid ? c.take<u32>(n) : nullptr;
  }
}
static void sort_sizes(Carver& c, size_t n, SortBufs& sb, bool payload) { sort_sizes(c, n, sb, payload, payload); }

// (sort key, one payload column), no row ids: B of SEMI / ANTI and of their predicate form, the pairs of an aggregate,
// plain MERGE
static void sort_sizes_key_payload(Carver& c, size_t n, SortBufs& sb) { sort_sizes(c, n, sb, true, false); }

// (sort key, row id), no end column: the event keys of DISJOIN and of the coverage segments
static void sort_sizes_key_rid(Carver& c, size_t n, SortBufs& sb) { sort_sizes(c, n, sb, false, true); }

// two keys-only sorts of one side, its starts and its ends: B of COUNT and of COUNT over DISTANCE
static void sort_sizes_starts_ends(Carver& c, size_t n, SortBufs& sstart, SortBufs& send) {
  for (int k = 0; k < 2; k++) {
    sstart.key[k] = c.take<u32>(n);
    sstart.end[k] = sstart.rid[k] = nullptr;
    send.key[k] = c.take<u32>(n);
    send.end[k] = send.rid[k] = nullptr;
  }
}

// Fork / join of the context's second stream.  A side of a few million rows is a chain of ~10 launches
// of 10-40 us each that do not fill the GPU (look-back latency, not bandwidth, bounds them): run beside
// the other side's chain it costs almost nothing.  Work given to stream() is ordered after everything
// already on the caller's stream; join() orders the caller's stream after it.  A call that returns
// early (an error) synchronises the second stream in the destructor, so no kernel outlives the arena.
struct SideChain {
  giql_hip_ctx* ctx;
  hipStream_t main;
  bool active = false, joined = false;
  // n_small: rows of the side given to the second stream.  It must be small (<= OVERLAP_MAX_ROWS): its chain is then latency-bound and costs the other side's
  // kernels little (SEMI 1M x 10M: 0.378 -> 0.349 ms; 1M x 1M: 0.387 -> 0.351 ms).
  SideChain(giql_hip_ctx* c, hipStream_t m, size_t n_small) : ctx(c), main(m) {
    if (!c->side_stream || n_small == 0 || n_small > OVERLAP_MAX_ROWS) return;
    if (sort_is_local(sort_tuning(c), n_small)) return;  // the bucket sort's boundary / queue buffers are one per context
    if (hipEventRecord(c->ev_fork, m) != hipSuccess) return;
    if (hipStreamWaitEvent(c->side_stream, c->ev_fork, 0) != hipSuccess) return;
    active = true;
  }
  hipStream_t stream() const { return active ? ctx->side_stream : main; }
  int join() {
    if (active && !joined) {
      joined = true;
      HIP_TRY(hipEventRecord(ctx->ev_join, ctx->side_stream));
      HIP_TRY(hipStreamWaitEvent(main, ctx->ev_join, 0));
    }
    return GIQL_OK;
  }
  ~SideChain() {
    if (active && !joined) (void)hipStreamSynchronize(ctx->side_stream);
  }
};

// A call returns this (internal, never across the C ABI) when one of the context's guesses turned out wrong at its
// read-back: its result is not valid, the guess has been dropped (set from what the read-back showed), and
// with_order_fallback repeats the call.  Each repeat runs with one guess fewer, so a call drops at most:
//   INNER plan / join: 1 -- the speculated form, layout, fused count, sorted inputs and join in the bucket stage are
//     all dropped together (spec_valid = false): the repeat reads the lengths back and speculates on nothing;
//   SEMI / ANTI / COUNT: 1 -- the fixed length of B (row_spec_valid = false): the repeat reads it back;
//   NEAREST k = 1: 2 -- the aligned layout (nearest_aligned = 0: the repeat builds no keys from the raw columns), then
//     the pile-ups (nearest_two_sorts = true, which also turns the layout off): the two-sort plan guesses nothing;
//   NEAREST k > 1, group_rows: 1 -- the pile-ups (nearest_two_sorts = true).
constexpr int GIQL_STATUS_GUESS_MISSED = -101;
constexpr int MAX_GUESS_MISSES = 2;

// The one loop that repeats a call:
//   a guess that missed (GIQL_STATUS_GUESS_MISSED): repeat, at most MAX_GUESS_MISSES times;
//   a bucket too large for the in-LDS stage (GIQL_STATUS_RESORT, bucket_sort.hip.h): this table wants the four-pass
//     sort -- for good on this context, so once;
//   a look-back timeout: belt and braces around the sort -- its look-back makes progress whatever the dispatch order
//     (blocks compute silent predecessors themselves, k_onesweep), so a timeout status is never expected; should one
//     be reported all the same, the call is repeated in the ticket order (order 0) and the context stays in it: once.
// Every attempt is a call of its own (its own prologue and guards); nothing of one attempt outlives it.
template <typename F>
static int with_order_fallback(giql_hip_ctx* ctx, F&& call) {
  int misses = 0;
  for (;;) {
    const int rc = call();
    if (rc == GIQL_STATUS_GUESS_MISSED) {
      if (++misses > MAX_GUESS_MISSES)
        return set_err(GIQL_ERR_STATE, "internal: more than %d guesses missed in one call", MAX_GUESS_MISSES);
      continue;
    }
    if (rc == GIQL_STATUS_RESORT && ctx && ctx->guess.local_sort) {
      ctx->guess.local_sort = false;
      ctx->guess.local_resorts++;
      misses = 0;  // (the guesses the failed attempt met are still in place: the repeat may drop them again)
      continue;
    }
    if (rc == GIQL_ERR_HIP && ctx && ctx->guess.os_order != 0 && ctx->h_meta && ctx->h_meta->status == GIQL_ERR_HIP) {
      ctx->guess.os_order = 0;
      ctx->guess.order_fallbacks++;
      misses = 0;
      continue;
    }
    return rc;
  }
}

// Fixed-length B side of the per-row operators: the canonical length every B row has (all of
// them regular), else 0.  From the span pass's length range.
static inline i64 uniform_len_b(const DevMeta& m) {
  return (m.len_min_b == m.len_max_b && m.len_max_b > 0) ? (i64)m.len_max_b : 0;
}

// Decide the form of a per-row operator after run_spans: a context that has run before assumes
// the previous call's answer (no stream sync here) and the caller validates it with
// row_form_settled() at the read-back the call ends with anyway; the first call reads the
// lengths back.
static int row_form_guess(giql_hip_ctx* ctx, hipStream_t st, i64& uni_len, bool& speculated) {
  uni_len = 0;
  speculated = false;
  if (ctx->sw.no_uniform) return GIQL_OK;
  if (ctx->guess.row_spec_valid) {
    uni_len = ctx->guess.row_spec_len;
    speculated = true;
    return GIQL_OK;
  }
  GIQL_TRY(read_meta(ctx, st));
  uni_len = uniform_len_b(*ctx->h_meta);
  ctx->guess.last_span = ctx->h_meta->total_span;  // known before anything is sorted: the sort form follows the real density
  return GIQL_OK;
}

// After the final read-back: remember the answer; false = the call assumed a fixed length that
// B does not have (its result is wrong: repeat it; the general form is right on any input, so a
// wrong "not fixed-length" guess only costs speed).
static bool row_form_settled(giql_hip_ctx* ctx, i64 uni_len, bool speculated) {
  if (ctx->sw.no_uniform) return true;
  const i64 actual = uniform_len_b(*ctx->h_meta);
  const bool ok = !(speculated && uni_len != 0 && actual != uni_len);
  ctx->guess.row_spec_valid = ok;
  ctx->guess.row_spec_len = actual;
  return ok;
}

// ------------------------------------------------------------- switches
static void parse_flag(const char* v, void* f) { *(bool*)f = atoi(v) != 0; }
static void parse_int(const char* v, void* f) { *(int*)f = atoi(v); }
static void parse_u32(const char* v, void* f) { *(u32*)f = (u32)strtoul(v, nullptr, 10); }
static void parse_classic(const char* v, void* f) { *(bool*)f = strcmp(v, "classic") == 0; }
static void parse_positive(const char* v, void* f) {
  if (atof(v) > 0) *(double*)f = atof(v);
}
static void parse_nonnegative(const char* v, void* f) {
  if (atof(v) >= 0) *(double*)f = atof(v);
}
static void parse_local_bits(const char* v, void* f) {
  if (atoi(v) >= BS_MIN_WBITS && atoi(v) <= 16) *(int*)f = atoi(v);
}
static void parse_local_min_rows(const char* v, void* f) {
  Switches& s = *(Switches*)f;
  s.local_min_rows = strtoull(v, nullptr, 10);
  s.local_max_bucket_rows = 1e30;  // a forced size threshold (tests, sweeps) is not second-guessed by density
  s.local_min_bucket_rows = 0.0;
}

static Switches read_switches() {
  Switches s;
  const struct {
    const char* name;
    void (*parse)(const char*, void*);
    void* field;
  } table[] = {
      {"GIQL_HIP_SORT", parse_classic, &s.classic_sort},
      {"GIQL_HIP_OS_VARIANT", parse_int, &s.os_variant},
      {"GIQL_HIP_OS_ORDER", parse_int, &s.os_order},
      {"GIQL_HIP_OS_HELP_AFTER", parse_u32, &s.os_help_after},
      {"GIQL_HIP_INJECT_TIMEOUT", parse_int, &s.inject_timeout},
      {"GIQL_HIP_NO_UNIFORM", parse_flag, &s.no_uniform},
      {"GIQL_HIP_NO_SPAN_HIST", parse_flag, &s.no_span_hist},
      {"GIQL_HIP_NO_COARSE_B", parse_flag, &s.no_coarse_b},
      {"GIQL_HIP_COARSE_MAX_GROUP_ROWS", parse_positive, &s.coarse_max_group_rows},
      {"GIQL_HIP_NO_FUSE_COUNT", parse_flag, &s.no_fuse_count},
      {"GIQL_HIP_NO_LOCAL_SORT", parse_flag, &s.no_local_sort},
      {"GIQL_HIP_LOCAL_MIN_ROWS", parse_local_min_rows, &s},  // (before the two bounds it lifts: they may be set too)
      {"GIQL_HIP_LOCAL_MIN_BUCKET_ROWS", parse_nonnegative, &s.local_min_bucket_rows},
      {"GIQL_HIP_LOCAL_MAX_BUCKET_ROWS", parse_positive, &s.local_max_bucket_rows},
      {"GIQL_HIP_NO_NARROW_BUCKETS", parse_flag, &s.no_narrow},
      {"GIQL_HIP_LOCAL_BITS", parse_local_bits, &s.force_bits},
  };
  for (const auto& row : table)
    if (const char* v = getenv(row.name)) row.parse(v, row.field);
  return s;
}

// ================================================================= C ABI
extern "C" {

int giql_hip_abi_version(void) { return GIQL_HIP_ABI_VERSION; }

const char* giql_hip_last_error(void) { return g_err; }

int giql_hip_device_count(int* n_devices) {
  if (!n_devices) return set_err(GIQL_ERR_INVALID, "n_devices is NULL");
  int n = 0;
  HIP_TRY(hipGetDeviceCount(&n));
  *n_devices = n;
  return GIQL_OK;
}

int giql_hip_create(int device, giql_hip_ctx** out) {
  if (!out) return set_err(GIQL_ERR_INVALID, "out is NULL");
  *out = nullptr;
  int n = 0;
  HIP_TRY(hipGetDeviceCount(&n));
  if (device < 0 || device >= n)
    return set_err(GIQL_ERR_INVALID, "device %d not in [0,%d)", device, n);
  HIP_TRY(hipSetDevice(device));
  giql_hip_ctx* ctx = new (std::nothrow) giql_hip_ctx(read_switches());
  if (!ctx) return set_err(GIQL_ERR_NOMEM, "out of host memory");
  ctx->device = device;
  memset(&ctx->stats, 0, sizeof(ctx->stats));
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
      ctx->n_cu = prop.multiProcessorCount;
  }
  bool ok = ctx->d_meta.alloc(sizeof(DevMeta)) == GIQL_OK &&
            hipHostMalloc((void**)&ctx->h_meta, sizeof(DevMeta), hipHostMallocDefault) == hipSuccess &&
            ctx->d_scratch64.alloc(64) == GIQL_OK;
  if (ok &&
      (hipStreamCreateWithFlags(&ctx->side_stream, hipStreamNonBlocking) != hipSuccess ||
       hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) != hipSuccess ||
       hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming) != hipSuccess))
    ctx->side_stream = nullptr;  // no second stream: everything stays on the caller's
  ok = ok && ctx->bucket_bnd.alloc(((size_t)BS_MAX_BUCKETS + 16) * sizeof(u32)) == GIQL_OK &&
       ctx->bucket_big.alloc(((size_t)BS_MAX_BUCKETS + 16) * sizeof(u32)) == GIQL_OK &&
       ctx->bucket_qwin.alloc(((size_t)2 * BS_MAX_BUCKETS + 16) * sizeof(u32)) == GIQL_OK;
  if (!ok) {
    const hipError_t e = hipGetLastError();  // (of the allocation that failed: nothing was called after it)
    giql_hip_destroy(ctx);
    return set_err(GIQL_ERR_HIP, "context allocation failed: %s", hipGetErrorString(e));
  }
  *out = ctx;
  return GIQL_OK;
}

int giql_hip_destroy(giql_hip_ctx* ctx) {
  if (!ctx) return GIQL_OK;
  (void)hipSetDevice(ctx->device);
  (void)hipDeviceSynchronize();
  for (auto e : ctx->ev_pool) (void)hipEventDestroy(e);
  if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
  if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
  if (ctx->side_stream) (void)hipStreamDestroy(ctx->side_stream);
  if (ctx->h_meta) (void)hipHostFree(ctx->h_meta);
  delete ctx;  // (the device buffers go with it)
  return GIQL_OK;
}

int giql_hip_reserve(giql_hip_ctx* ctx, int64_t bytes) {
  if (!ctx || bytes < 0) return set_err(GIQL_ERR_INVALID, "bad ctx/bytes");
  HIP_TRY(hipSetDevice(ctx->device));
  return ensure_arena(ctx, (size_t)bytes, nullptr);
}

int giql_hip_set_profiling(giql_hip_ctx* ctx, int enabled) {
  if (!ctx) return set_err(GIQL_ERR_INVALID, "ctx is NULL");
  if (enabled >= 16 && enabled < 16 + GIQL_PH_N) {  // events around ONE phase only: 16 + its GIQL_PH_* number
    ctx->profiling = 2;
    ctx->profile_phase = enabled - 16;
    return GIQL_OK;
  }
  ctx->profiling = enabled < 0 ? 0 : (enabled > 2 ? 1 : enabled);
  ctx->profile_phase = GIQL_PH_SORT_SCATTER;
  return GIQL_OK;
}

int giql_hip_get_stats(giql_hip_ctx* ctx, giql_hip_stats* out) {
  if (!ctx || !out) return set_err(GIQL_ERR_INVALID, "ctx/out is NULL");
  if (ctx->profiling && !ctx->spans.empty()) {
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipEventSynchronize(ctx->spans.back().b));
    collect_spans(ctx);
  }
  ctx->stats.workspace_bytes = (int64_t)ctx->arena.bytes();
  *out = ctx->stats;
  // byte 0: join form (+ bit 5: a side was sorted in three stages, bit 6: this context fell back to
  // the four-pass sort for good); byte 1: sort tile order in force; bits 16-26: order fallbacks so far; bits 27-28:
  // 16 - the key bits of the last bucket stage's buckets (0: 65,536-key buckets)
  out->reserved = (ctx->stats.reserved & 0x1F) | (ctx->call.last_sort_local ? 0x20 : 0) |
                  (ctx->guess.local_resorts ? 0x40 : 0) | (ctx->plan.swapped ? 0x80 : 0) | ((ctx->guess.os_order & 0x7F) << 8) |
                  (ctx->call.count_fused ? 0x8000 : 0) | ((ctx->call.used_sorted[0] || ctx->call.used_sorted[1]) ? (int32_t)0x80000000u : 0) |
                  ((ctx->guess.order_fallbacks & 0x7FF) << 16) | (((16 - ctx->call.last_local_bits) & 3) << 27) |
                  (ctx->call.bucket_join ? (1 << 29) : 0) |
                  (ctx->plan.fuse_done ? (1 << 30) : 0);
  return GIQL_OK;
}

// ------------------------------------------------------------------ INNER
// One side of an INNER plan (A or B in the plan's labels): everything a side owns, bound once in inner_plan_core.  The
// forms take the two sides by ROLE -- query / sorted (Q, U) in the fixed-length form, A / B in the general one -- and
// never select between "the A one" and "the B one" themselves.
struct PlanSide {
  const giql_side* side = nullptr;
  size_t n = 0;
  int label = 0;             // 0 = A, 1 = B: run_linearize, DevMeta's per-side fields, guess.spec_sorted
  SortBufs* sort = nullptr;  // inside InnerState: the sorted (key, end, rid) stay for inner_fill
  u32 *hist = nullptr, *gbase = nullptr;  // digit histogram replicas / digit offsets of its sort
  u32* status = nullptr;     // its sort's status words (bind_status)
  u32* irr_list = nullptr;
  const u32* irr = nullptr;      // DevMeta: its irregular rows
  const int* len_max = nullptr;  // DevMeta: its longest regular row
  int32_t* out_row = nullptr;    // one-call join: the caller's output row for this side's ids (else NULL)
  Side which() const { return label ? Side::B : Side::A; }
  DigitCounts starts() const { return {hist, gbase}; }
  SortRequest sort_rows() const { return SortRequest::rows((u32)n, gbase, status); }
};

// The plan's scratch, as carve_inner lays it out in the arena.
struct InnerScratch {
  LinBufs lb;
  u32 *tile_hist = nullptr, *irr_cnt = nullptr, *top_partial_q = nullptr;
  u32 *hist[2] = {nullptr, nullptr}, *gbase[2] = {nullptr, nullptr};  // [label]
  u32 *os_status = nullptr, *os_status2 = nullptr;  // status words: the larger side's, the smaller side's
  u64 *bsums = nullptr, *bsums1 = nullptr, *scan_chain = nullptr;
  ZeroSpan zero;  // what is zeroed up front, less the larger side's status words that follow it (zero_inner_scratch)
};

// What ONE attempt at a plan assumed.  begin_attempt fills the upper part right after the span pass; the forms add the
// choices that depend on sizes; settle_guesses checks all of it against the final read-back.  The stages read these
// fields, they do not derive them again.
struct InnerAttempt {
  bool onesweep = false;
  int big_side = 0;          // the larger side's label: the one the fixed-length form prefers as its sorted side
  bool speculated = false;   // form, layout and the guesses below come from the context's previous plan, not from a read-back
  int form = 0;              // 0 general, 1 B fixed-length (queries = A rows), 2 A fixed-length
  i64 uni_len = 0;
  bool want_hist = false;    // the larger side's span pass counted the digits of its aligned keys
  bool want_hist_q = false;  // ... and the other side's too
  bool aligned = false;      // the aligned layout holds (a guess when speculated)
  bool keygen_u = false;     // fixed-length form: the sorted side is sorted straight from its raw columns
  bool keygen_q = false;     // ... and the query side too (on no_irr)
  bool keygen_g = false;     // general form: the larger side is (on no irregular row IN IT)
  bool presorted[2] = {false, false};  // [label] the side arrives in (chrom id, start) order: its sort is skipped
  bool no_irr = false;       // guess.last_no_irr as used: speculated, and the previous plan met no irregular row
  bool fuse_len_ok = false;  // no query row longer than the fused windows allow for
  // chosen by the forms
  int q_skip = 0;            // low digits the query side's sort left out (on no_irr)
  bool fuse_cnt = false;     // the sorted side's bucket stage answers the queries' bounds
  bool early_fill = false;   // the fill is launched inside the plan
  bool join_in_buckets = false;  // fixed-length form: the bucket stage writes the pairs (FUSE == 2)
  bool general_join = false;     // general form: the same (FUSE == 3)

  bool count_fused() const { return fuse_cnt || general_join; }
  bool bucket_join() const { return join_in_buckets || general_join; }
};

static inline int len_min_of(const DevMeta& m, int label) { return label ? m.len_min_b : m.len_min_a; }
static inline int len_max_of(const DevMeta& m, int label) { return label ? m.len_max_b : m.len_max_a; }
static inline u32 skip_mask(int q_skip) { return q_skip == 2 ? 0xFFFF0000u : (q_skip == 1 ? 0xFFFFFF00u : 0xFFFFFFFFu); }

// Uniform-length side?  (fixed-length reads: min == max canonical length > 0 over ALL its rows; a single irregular
// row makes the minimum 0.)  The form follows from the length ranges of the span pass.
static void decide_form(const DevMeta& m, size_t na, size_t nb, bool no_uniform, int& form, i64& len) {
  const bool ub = m.len_min_b == m.len_max_b && m.len_max_b > 0;
  const bool ua = m.len_min_a == m.len_max_a && m.len_max_a > 0;
  form = 0;
  len = 0;
  if (no_uniform) return;  // GIQL_HIP_NO_UNIFORM: the general form whatever the lengths
  // sort the uniform side without its end; prefer the larger side when both are
  if (ub && (!ua || nb >= na)) {
    form = 1;
    len = m.len_max_b;
  } else if (ua) {
    form = 2;
    len = m.len_max_a;
  }
}

// the fused count's windows allow for query rows up to BS_FUSE_WCAP long (general form: both sides' rows)
static bool fuse_len_ok(const DevMeta& m, int form) {
  if (form != 0) return len_max_of(m, form == 1 ? 0 : 1) <= (int)BS_FUSE_WCAP;
  return m.len_max_a <= (int)BS_FUSE_WCAP && m.len_max_b <= (int)BS_FUSE_WCAP;
}

// The arena layout of a plan.  (The order and sizes of the take<> calls are public through stats.workspace_bytes, and
// the single up-front memset depends on the order.)
static size_t carve_inner(giql_hip_ctx* ctx, char* base, size_t na, size_t nb, int n_chrom, bool onesweep,
                          InnerScratch& W) {
  InnerState& S = ctx->plan.inner;
  const size_t nq = na + nb, n_max = na > nb ? na : nb;
  const size_t n_tiles_max = cdiv(n_max, RS_TILE);
  const size_t scan_max = (nq > n_tiles_max * RS_BINS ? nq : n_tiles_max * RS_BINS);
  constexpr u32 TQ2 = RC_NT * RC_ITEMS_C2;
  Carver c{base};
  common_sizes(c, n_chrom, W.lb);
  sort_sizes(c, na, S.sa, true);
  sort_sizes(c, nb, S.sb, true);
  if (onesweep) {
    // everything that has to start at zero lies back to back, the larger side's status words last: ONE memset
    // up front instead of one per histogram and per sort (5 launches of ~5 us at the headline sizes)
    c.open_zeroed();
    W.hist[0] = c.take<u32>((size_t)LIN_HIST_REPLICAS * 1024);
    W.hist[1] = c.take<u32>((size_t)LIN_HIST_REPLICAS * 1024);
    W.lb.top_partial = c.take<u32>((size_t)LIN_HIST_REPLICAS * MM_TOP_WORDS);
    W.top_partial_q = c.take<u32>((size_t)LIN_HIST_REPLICAS * MM_TOP_WORDS);
    W.gbase[0] = c.take<u32>(1024);
    W.gbase[1] = c.take<u32>(1024);
    W.lb.abase = c.take<u32>(MM_HIST_CHROMS);
    W.os_status2 = c.take<u32>(4 * os_pass_words(na < nb ? na : nb));  // the smaller side's
    W.zero = c.close_zeroed();
    W.os_status = c.take<u32>(4 * os_pass_words(n_max));               // the larger side's
  } else {
    W.tile_hist = c.take<u32>(n_tiles_max * RS_BINS);
  }
  W.bsums = c.take<u64>(cdiv(scan_max, SCAN_TILE) + 2);
  S.wlo1 = c.take<u32>((size_t)S.nt1 + 2 + (S.c1_fill ? cdiv(nb, TQ2) : 0));
  S.c1_base = c.take<u64>((size_t)S.nt1 + 2);
  const size_t n1 = S.c1_fill ? nb : 0;
  S.lo1 = c.take<u32>(n1);
  S.cnt1 = c.take<u32>(n1);
  S.off1 = c.take<u64>(n1 + 1);
  W.bsums1 = c.take<u64>(cdiv(n1 ? n1 : 1, SCAN_TILE) + 2);
  const size_t nq2 = ctx->sw.no_uniform ? na : n_max;  // the uniform form may query the other side
  S.wlo2 = c.take<u32>((size_t)cdiv(nq2, TQ2) + 2);
  S.cnt2 = c.take<u32>(nq2);
  S.lo2 = c.take<u32>(nq2);
  S.off2 = c.take<u64>(nq2 + 1);
  W.scan_chain = c.take<u64>((size_t)cdiv(nq2, SCAN_TILE) + 4);  // chained scan: a status word per tile + the ticket
  ctx->plan.irr_a_list = c.take<u32>(na);
  ctx->plan.irr_b_list = c.take<u32>(nb);
  W.irr_cnt = c.take<u32>(nq);
  ctx->plan.irr_off = c.take<u64>(nq + 1);
  return c.off;
}

// The one place that knows how many passes of the larger side's status words are zeroed.  First call: the whole zero
// span and those passes in ONE memset (the larger side takes at most 4 passes, 2 or 3 in the three-stage form).  Later
// calls: the larger side turned out to take more global passes than expected (the density is known now): those need
// zeroed status words too, and the zeroed range grows by them.
static int zero_inner_scratch(giql_hip_ctx* ctx, hipStream_t st, const InnerScratch& W, size_t n_max) {
  const SortTuning tune = sort_tuning(ctx);
  const int passes = sort_is_local(tune, n_max) ? local_passes(sort_local_bits(tune, n_max)) : 4;
  const size_t want = W.zero.end + (size_t)passes * os_pass_stride(tune, n_max) * sizeof(u32);  // (os_status starts at zero.end)
  const char* const arena = ctx->arena;
  const char* const have = ctx->call.zeroed.end();  // (nothing to do when the range reaches that far already)
  return zero_span(ctx, st, {have ? (size_t)(have - arena) : W.zero.off, want});
}

// (the smaller side's passes use the smaller status buffer: both were zeroed up front, neither is reused; of two
// sides of equal size, `x` takes it)
static void bind_status(const InnerScratch& W, PlanSide& x, PlanSide& y) {
  const bool x_small = x.n <= y.n;
  x.status = x_small ? W.os_status2 : W.os_status;
  y.status = x_small ? W.os_status : W.os_status2;
}

// The span pass, and what this attempt assumes from here on.
//
// The larger side is the one the uniform form prefers as its fixed-length side: its span pass also counts the
// digits of its keys (aligned layout), so that, if the form and the layout hold, it is sorted straight from its raw
// columns with no linearize pass.  A context that has planned before asks for it only when its last plan ended that
// way.
//
// The form is decided from the length ranges the min/max pass produces.  Reading them back costs a stream sync in
// the middle of the plan (one 100-byte readback; it also surfaces chrom / span errors before the sort), so a context
// that has planned before SPECULATES on its previous decision and validates it against the same numbers at the
// read-back the plan ends with anyway (settle_guesses); a wrong guess (the kernels are memory-safe on any input)
// repeats the plan once without speculation.
static int begin_attempt(giql_hip_ctx* ctx, hipStream_t st, PlanSide& A, PlanSide& B, int n_chrom, InnerScratch& W,
                         InnerAttempt& T) {
  const Guesses& g = ctx->guess;
  PlanSide& big = T.big_side ? B : A;
  PlanSide& other = T.big_side ? A : B;
  const int big_form = T.big_side ? 1 : 2;  // the fixed-length form whose sorted side is the larger one
  T.speculated = T.onesweep && g.spec_valid;
  T.no_irr = T.speculated && g.last_no_irr;
  T.want_hist = T.onesweep && !ctx->sw.no_span_hist && ctx->sw.os_variant == 0 && n_chrom <= MM_HIST_CHROMS;
  if (T.want_hist && T.speculated)  // ... or in the general form without irregular rows (its larger side)
    T.want_hist = g.spec_aligned && (g.spec_form == big_form || (g.spec_form == 0 && g.last_no_irr));
  // ... and the QUERY side of the fixed-length form too (round 3): its (key, end, rid) sort starts from the raw
  // columns as well (k_onesweep<3, .., KEYGEN>), so neither side has a linearize pass -- on the guesses that the
  // form and the layout hold AND that the query side has no irregular row (those carry the sentinel key and a
  // list entry, which only the linearize pass produces): validated at the read-back like the others.
  T.want_hist_q = T.want_hist && T.no_irr && g.spec_form == big_form && other.n > 0;
  if (T.want_hist_q) {
    W.lb.hist_partial2 = other.hist;
    W.lb.top_partial2 = W.top_partial_q;
  }
  GIQL_TRY(run_spans(ctx, st, *A.side, *B.side, n_chrom, W.lb, T.want_hist ? T.big_side : -1, big.hist));
  if (T.speculated) {
    T.form = g.spec_form;
    T.uni_len = g.spec_len;
    T.aligned = T.want_hist;  // = g.spec_aligned when the form matches
    T.fuse_len_ok = g.spec_fuse_len_ok;
    // Sorted inputs: a side the span pass found in (chrom id, start) order (and free of irregular rows) skips its
    // sort -- from the read-back on a first plan, the previous plan's answer afterwards (validated in settle_guesses)
    T.presorted[0] = g.spec_sorted[0];
    T.presorted[1] = g.spec_sorted[1];
  } else if (T.onesweep) {
    GIQL_TRY(read_meta(ctx, st));
    const DevMeta& m = *ctx->h_meta;
    decide_form(m, A.n, B.n, ctx->sw.no_uniform, T.form, T.uni_len);
    T.aligned = T.want_hist && m.aligned_ok != 0;
    T.fuse_len_ok = fuse_len_ok(m, T.form);
    T.presorted[0] = m.unsorted_a == 0;
    T.presorted[1] = m.unsorted_b == 0;
    // the span is known now, before anything is sorted: the sort form follows the table's real density
    // already on this first plan (the one write of a guess outside settle_guesses).  The span pass counted its
    // digits for the form it expected: if the larger side leaves the three-stage sort, its high-digits-only
    // histogram is of no use and that side is linearized (which counts all four digits)
    const int expected_bits = sort_local_bits(sort_tuning(ctx), big.n);  // by the previous call's density ...
    ctx->guess.last_span = m.total_span;
    // (the high-digits-only histogram serves 16-bit buckets alone: narrower ones sort on bits 8-15 too)
    if (expected_bits == 16 && sort_local_bits(sort_tuning(ctx), big.n) != 16) T.aligned = false;  // ... and by this one's
    GIQL_TRY(zero_inner_scratch(ctx, st, W, big.n));
  }
  T.keygen_u = T.aligned && T.form == big_form;
  T.keygen_q = T.keygen_u && T.want_hist_q;
  // General form: the larger side's (key, end, rid) sort can start from the raw columns too, as long as
  // that side holds no irregular row (those carry the sentinel key, which depends on `end`; the span pass
  // counted digits of start alone).  Known from the read-back on a first plan, a guess afterwards.
  T.keygen_g = T.aligned && T.form == 0 && (T.speculated ? g.last_no_irr : len_min_of(*ctx->h_meta, T.big_side) > 0);
  return GIQL_OK;
}

// The span pass counted a side's digits already: fold the per-chromosome top digits onto the bases and scan, and let
// the first sort pass build the keys from (chrom, start) -- no linearize pass.  hist2 / gbase2: the other side's as
// well (lb.top_partial2), both in one launch pair.
static int span_digit_offsets(giql_hip_ctx* ctx, hipStream_t st, const LinBufs& lb, u32* hist, u32* gbase,
                              u32* hist2, u32* gbase2, const char* what) {
  Phase ph(ctx, st, GIQL_PH_LINEARIZE, 2);
  if (hist2) {
    hipLaunchKernelGGL(k_fold_top2, dim3(MM_HIST_CHROMS, 2), dim3(256), 0, st, lb.top_partial, lb.top_partial2,
                       lb.abase, hist, hist2);
    hipLaunchKernelGGL(k_digit_offsets2, dim3(4, 2), dim3(256), 0, st, hist, hist2, (u32)LIN_HIST_REPLICAS, gbase,
                       gbase2);
  } else {
    hipLaunchKernelGGL(k_fold_top, dim3(MM_HIST_CHROMS), dim3(256), 0, st, lb.top_partial, lb.abase, hist);
    hipLaunchKernelGGL(k_digit_offsets, dim3(4), dim3(256), 0, st, hist, (u32)LIN_HIST_REPLICAS, gbase);
  }
  return post_launch(what);
}

// The query side of a fused bucket stage as its own sort left it, and where a join writes its pairs.
struct FuseQuery {
  const SortBufs* sort;
  size_t n;
  const u32* irr;      // rows of it that match nothing (sorted last, skipped by the windows)
  const u32* gbase;    // its sort's digit offsets
  const int* len_max;  // device: its longest row
};
struct FuseTarget {
  int32_t *row_q, *row_s;
  u64 cap;
};
static inline FuseQuery fuse_query(const PlanSide& q) { return FuseQuery{q.sort, q.n, q.irr, q.gbase, q.len_max}; }

// The FuseCount of a bucket stage: bounds only (join == NULL; the caller adds its outputs: dev.lo_out / hi_out and the
// words to zero), or the join itself, with the pairs counted in DevMeta::n_out (zeroed by the span pass / by
// k_init_minmax).  general: rows of any length on both sides; len_max_u = how far the windows then reach up.
static FuseCount make_fuse_count(giql_hip_ctx* ctx, const FuseQuery& q, i64 lo_off, u32 key_mask,
                                 const FuseTarget* join, bool general, const int* len_max_u, u32* zero_ptr) {
  FuseCount fc = {};  // (no bounds outputs, no words to zero, no pairs target unless set below)
  fc.join = join != nullptr;
  fc.general = general;
  fc.zero_ptr = zero_ptr;
  fc.dev.qkey = q.sort->key[0];
  fc.dev.qend = q.sort->end[0];
  fc.dev.qwin = ctx->bucket_qwin;
  fc.dev.lo_off = lo_off;
  if (join) {
    fc.dev.qrid = q.sort->rid[0];
    fc.dev.row_q = join->row_q;
    fc.dev.row_s = join->row_s;
    fc.dev.cap = join->cap;
    fc.dev.cursor = reinterpret_cast<unsigned long long*>(&ctx->d_meta->n_out);
  }
  fc.nq_total = (u32)q.n;
  fc.irr_q = q.irr;
  fc.gbq3 = q.gbase + 3 * OS_BINS;
  fc.key_mask = key_mask;
  fc.len_max_q = q.len_max;
  fc.len_max_u = general ? len_max_u : nullptr;
  return fc;
}

// The bucket stage wrote the pairs, counted in DevMeta::n_out: read the count back; the join stands only if every
// guess held and the pairs fitted.
static int finish_bucket_join(giql_hip_ctx* ctx, hipStream_t st) {
  GIQL_TRY(read_meta(ctx, st));
  ctx->plan.n_c1 = 0;
  ctx->plan.n_reg = ctx->h_meta->n_out;
  ctx->plan.fuse_done = ctx->h_meta->irr_a + ctx->h_meta->irr_b == 0 && ctx->plan.n_reg <= ctx->plan.fuse_cap;
  ctx->stats.phase_bytes[GIQL_PH_SORT_LOCAL] += (int64_t)8 * (int64_t)ctx->plan.n_reg;  // the pairs
  return GIQL_OK;
}

// ---- uniform-length form: queries Q (full rows) against points U (starts only)
static int plan_uniform(giql_hip_ctx* ctx, hipStream_t st, int n_chrom, PlanSide& Q, PlanSide& U, InnerScratch& W,
                        InnerAttempt& T) {
  InnerState& S = ctx->plan.inner;
  const LinBufs& lb = W.lb;
  SortBufs& sq = *Q.sort;
  SortBufs& su = *U.sort;
  su.end[0] = su.end[1] = nullptr;  // the uniform side carries (key, rid) only
  bind_status(W, Q, U);
  // Fused range count: when U takes the three-stage sort, its bucket sort answers the queries' bounds
  // (bucket_sort.hip.h) -- as long as no query row is longer than the windows allow for: known from the
  // read-back on a first plan, the previous plan's answer afterwards (validated like the other guesses)
  const SortTuning tune = sort_tuning(ctx);  // (the density guess is settled before a form runs)
  T.fuse_cnt = !ctx->sw.no_fuse_count && sort_is_local(tune, U.n) && T.fuse_len_ok;
  // KNOWN ODDITY (kept as it is): on a speculated attempt this is not the previous INNER plan's maximum but the last
  // read-back of ANY call on the context (h_meta is shared); it only sizes the window estimate below.
  const int q_len_max = len_max_of(*ctx->h_meta, Q.label);
  if (T.keygen_u) {
    // (the query side sorted from its raw columns too: its digits were counted in the span pass)
    GIQL_TRY(span_digit_offsets(ctx, st, lb, U.hist, U.gbase, T.keygen_q ? Q.hist : nullptr, Q.gbase,
                                "digit offsets (span histogram)"));
  }
  // the query side's chain (linearize + sort) beside the other side's when it is small (the fused count
  // needs the sorted queries before U's last stage: one stream)
  // (the fork comes AFTER the digit offsets above: the query side's sort on the second stream reads them)
  SideChain sc(ctx, st, (Q.n <= U.n && !T.fuse_cnt) ? Q.n : 0);
  if (!T.keygen_q) {
    GIQL_TRY(run_linearize(ctx, sc.stream(), *Q.side, n_chrom, lb, Q.which(),
                           LinTarget::keys_ends(sq.key[0], sq.end[0], Q.irr_list), LinOptions().counting_starts(Q.starts())));
  }
  if (!T.keygen_u) {
    // uniform => no irregular row: `end` is not read
    GIQL_TRY(run_linearize(ctx, st, *U.side, n_chrom, lb, U.which(), LinTarget::keys_only(su.key[0], U.irr_list),
                           LinOptions().counting_starts(U.starts()).without_end_column()));
  }
  // The query side's order only serves locality (its bounds are searched per row, its pairs are laid
  // out by the scan), so its lowest digit stays unsorted: three passes.  Irregular rows would break
  // that (their sentinel keys must end up LAST, after every row of the top 256-key block): taken
  // only on the context's guess that there are none, validated with the other guesses.
  // With the fused count the queries only have to be grouped by the bucket their key falls into (the windows
  // of k_bucket_bounds_fused are computed under the same mask and then cover whole query buckets): TWO digits
  // unsorted, two passes.
  T.q_skip = (T.no_irr && !sort_is_local(tune, Q.n)) ? 1 : 0;
  // (narrower buckets: the queries stay grouped by key >> 8 -- a window under the 16-bit mask would span 2-8 buckets)
  const int wb_u = sort_local_bits(tune, U.n);
  if (T.q_skip && T.fuse_cnt && wb_u == 16) T.q_skip = 2;
  const u32 q_mask = skip_mask(T.q_skip);
  GIQL_TRY(run_sort_onesweep(ctx, sc.stream(), sq,
                             Q.sort_rows().keys_from(T.keygen_q ? Q.side : nullptr, lb.abase).skipping_digits(T.q_skip)
                                 .already_sorted(T.presorted[Q.label])));
  // One-call join (giql_hip_inner_join_dev): the caller's buffers are here and everything about this plan is a
  // guess that has held so far (same form as last time, no irregular rows), so the fill is launched inside the
  // plan, with a grid bounded by the capacity and the true count read on the device.
  constexpr u32 T2 = FILL_NT * FILL_ITEMS_C2;
  static_assert((T2 & (T2 - 1)) == 0, "fill tiles are a power of two (k_scan_chain_diff shifts)");
  const u64 nt_cap64 = (ctx->plan.fuse_cap + T2 - 1) / T2;
  const bool offered = Q.out_row && T.no_irr && ctx->plan.fuse_cap > 0;
  T.early_fill = offered && nt_cap64 <= 0x7FFFFFF0ull && ((size_t)nt_cap64 + 2) * sizeof(u32) <= ctx->part.bytes();
  // ... and, when the other side's bucket stage answers the bounds anyway, the pairs are written right there
  // (bucket_sort.hip.h, FUSE == 2) -- as long as the query windows stay well inside what a block holds in
  // registers: a window covers the query buckets (coarsely grouped: whole 65536-key buckets) that a bucket's
  // reach -- its own 65536 keys, the fixed length above it, the longest query below it -- touches
  const double win_keys = T.q_skip == 2 ? 3.0 * 65536.0 + (double)T.uni_len
                                        : (double)(1u << (wb_u ? wb_u : 16)) + 512.0 + (double)T.uni_len +
                                              (double)(q_len_max > 0 ? q_len_max : 0);
  T.join_in_buckets = T.fuse_cnt && offered && ctx->guess.last_span > 0 &&
                      (double)Q.n * win_keys / (double)ctx->guess.last_span <= 0.75 * (double)BJ_WCAP;
  FuseCount fc = {};
  if (T.fuse_cnt) {
    const FuseTarget out{Q.out_row, U.out_row, ctx->plan.fuse_cap};
    // u.start in [q.start - L + 1, q.end)
    fc = make_fuse_count(ctx, fuse_query(Q), 1 - T.uni_len, q_mask, T.join_in_buckets ? &out : nullptr, false, nullptr,
                         reinterpret_cast<u32*>(W.scan_chain));
    fc.zero_words = (u32)(2 * (cdiv(Q.n, SC_TILE) + 2));
    fc.dev.lo_out = S.lo2;
    fc.dev.hi_out = S.cnt2;  // the scan below turns the upper bounds into counts in place
  }
  GIQL_TRY(run_sort_onesweep(ctx, st, su,
                             U.sort_rows().keys_from(T.keygen_u ? U.side : nullptr, lb.abase)
                                 .fused_with(T.fuse_cnt ? &fc : nullptr).already_sorted(T.presorted[U.label])));
  GIQL_TRY(sc.join());
  constexpr u32 TQ = RC_NT * RC_ITEMS_C2;
  S.nt2 = cdiv(Q.n, TQ);
  if (T.join_in_buckets) return finish_bucket_join(ctx, st);
  bool part_done = false;  // the scan wrote the fill's partition
  if (T.fuse_cnt) {
    u32 log2_t2 = 0;
    while ((1u << log2_t2) < T2) log2_t2++;
    GIQL_TRY(run_scan_chain(ctx, st, GIQL_PH_SCAN, S.cnt2, S.lo2, Q.n, Q.irr, S.off2, W.scan_chain,
                            &ctx->d_meta->n_out, T.early_fill ? ctx->part : nullptr, log2_t2, (u32)nt_cap64 + 1));
    part_done = T.early_fill;
  } else {
    {
      Phase ph(ctx, st, GIQL_PH_COUNT, 2);
      const i64 lo_off = 1 - T.uni_len;  // u.start in [q.start - L + 1, q.end)
      hipLaunchKernelGGL(k_count_partition, dim3(cdiv((u64)S.nt2 + 1, 256)), dim3(256), 0, st,
                         sq.key[0], (u32)Q.n, Q.irr, su.key[0], (u32)U.n, U.irr, lo_off, TQ, S.nt2,
                         S.wlo2, q_mask);
      hipLaunchKernelGGL((k_range_count<RC_ITEMS_C2, RC_LDS_CAP>), dim3(S.nt2), dim3(RC_NT), 0, st,
                         sq.key[0], sq.end[0], (u32)Q.n, Q.irr, su.key[0], (u32)U.n, U.irr, lo_off,
                         S.wlo2, S.lo2, S.cnt2);
      GIQL_TRY(post_launch("range count (uniform)"));
    }
    GIQL_TRY(run_scan<u64>(ctx, st, GIQL_PH_SCAN, S.cnt2, Q.n, S.off2, W.bsums, S.off2 + Q.n, &ctx->d_meta->n_out));
  }
  if (T.early_fill) {
    // The early fill: no stream sync between plan and fill.  Validated at the read-back below and in
    // settle_guesses; a wrong guess leaves the buffers to the ordinary fill.
    const u32 nt_cap = (u32)nt_cap64;
    if (!part_done) {
      Phase ph(ctx, st, GIQL_PH_PARTITION);
      hipLaunchKernelGGL(k_partition, dim3(cdiv((u64)nt_cap + 1, 256)), dim3(256), 0, st, S.off2,
                         (u32)Q.n, (u64)0, T2, nt_cap, ctx->part, (const u64*)(S.off2 + Q.n), ctx->plan.fuse_cap);
    }
    {
      Phase ph(ctx, st, GIQL_PH_FILL);
      hipLaunchKernelGGL((k_fill<FILL_ITEMS_C2>), dim3(nt_cap), dim3(FILL_NT), 0, st, S.off2, S.lo2, sq.rid[0],
                         (u32)Q.n, su.rid[0], ctx->part, (u64)0, (u64)0, Q.out_row, U.out_row,
                         (const u64*)(S.off2 + Q.n), ctx->plan.fuse_cap);
    }
    GIQL_TRY(post_launch("fused fill"));
  }
  GIQL_TRY(read_meta(ctx, st));
  ctx->plan.n_c1 = 0;
  ctx->plan.n_reg = ctx->h_meta->n_out;
  // the early fill stands only if every guess held and the pairs fitted
  ctx->plan.fuse_done = T.early_fill && ctx->h_meta->irr_a + ctx->h_meta->irr_b == 0 && ctx->plan.n_reg <= ctx->plan.fuse_cap;
  return GIQL_OK;
}

// ---- general form: two classes of pairs -- class 1: a.start in [b.start, b.end), counted per B row against the
// sorted A starts; class 2: b.start in (a.start, a.end), counted per A row against the sorted B starts
// The general two-class form's counts and scans over the sorted sides (buffer 0 of sa / sbb), shared by plan_general and
// the within-distance plan: class 1 on `st1` (queries = sorted B over the sorted A starts), class 2 on `st` (queries =
// sorted A over the sorted B starts); totals land in DevMeta::n_out_c1 / n_out.  Which class-1 kernels run follows
// S.c1_fill / S.c1_items exactly as giql_hip_inner_fill_dev reads them back -- ONE copy, so the pairing cannot drift.
static int run_class_counts(giql_hip_ctx* ctx, InnerState& S, InnerScratch& W, SortBufs& sa, SortBufs& sbb, size_t na,
                            size_t nb, const u32* irr_a, const u32* irr_b, hipStream_t st1, hipStream_t st) {
  constexpr u32 TQ2 = RC_NT * RC_ITEMS_C2;
  {
    Phase ph(ctx, st, GIQL_PH_COUNT, 4);
    // class 1: queries = sorted B, points = sorted A starts, range [b.start, b.end);
    // only one total per block is kept (see k_c1_count)
    if (S.c1_fill) {
      const u32 nt1r = cdiv(nb, TQ2);
      hipLaunchKernelGGL(k_count_partition, dim3(cdiv((u64)nt1r + 1, 256)), dim3(256), 0, st1,
                         sbb.key[0], (u32)nb, irr_b, sa.key[0], (u32)na, irr_a, (i64)0, TQ2, nt1r, S.wlo1);
      hipLaunchKernelGGL((k_range_count<RC_ITEMS_C2, RC_LDS_CAP>), dim3(nt1r), dim3(RC_NT), 0, st1,
                         sbb.key[0], sbb.end[0], (u32)nb, irr_b, sa.key[0], (u32)na, irr_a, (i64)0, S.wlo1,
                         S.lo1, S.cnt1);
    } else {
      const u32 c1_tq = (u32)(C1_NT * S.c1_items);  // class-1 rows per block
      hipLaunchKernelGGL(k_count_partition, dim3(cdiv((u64)S.nt1 + 1, 256)), dim3(256), 0, st1,
                         sbb.key[0], (u32)nb, irr_b, sa.key[0], (u32)na, irr_a, (i64)0, c1_tq, S.nt1,
                         S.wlo1);
      if (S.c1_items == 2)
        hipLaunchKernelGGL(k_c1_count<2>, dim3(S.nt1), dim3(C1_NT), 0, st1, sbb.key[0], sbb.end[0], (u32)nb,
                           irr_b, sa.key[0], (u32)na, irr_a, S.wlo1, S.c1_base);
      else
        hipLaunchKernelGGL(k_c1_count<C1_ITEMS_MAX>, dim3(S.nt1), dim3(C1_NT), 0, st1, sbb.key[0], sbb.end[0], (u32)nb,
                           irr_b, sa.key[0], (u32)na, irr_a, S.wlo1, S.c1_base);
      // class-1 block totals -> block bases (one block, in place); total -> n_out_c1
      hipLaunchKernelGGL(k_scan_spine, dim3(1), dim3(1024), 0, st1, S.c1_base, S.nt1,
                         &ctx->d_meta->n_out_c1);
    }
    // class 2: queries = sorted A, points = sorted B starts, range (a.start, a.end)
    hipLaunchKernelGGL(k_count_partition, dim3(cdiv((u64)S.nt2 + 1, 256)), dim3(256), 0, st,
                       sa.key[0], (u32)na, irr_a, sbb.key[0], (u32)nb, irr_b, (i64)1, TQ2, S.nt2, S.wlo2);
    hipLaunchKernelGGL((k_range_count<RC_ITEMS_C2, RC_LDS_CAP>), dim3(S.nt2), dim3(RC_NT), 0, st,
                       sa.key[0], sa.end[0], (u32)na, irr_a, sbb.key[0], (u32)nb, irr_b, (i64)1, S.wlo2,
                       S.lo2, S.cnt2);
    GIQL_TRY(post_launch("range count"));
  }
  if (S.c1_fill) {
    GIQL_TRY(run_scan<u64>(ctx, st1, GIQL_PH_SCAN, S.cnt1, nb, S.off1, W.bsums1, S.off1 + nb, &ctx->d_meta->n_out_c1));
  }
  GIQL_TRY(run_scan<u64>(ctx, st, GIQL_PH_SCAN, S.cnt2, na, S.off2, W.bsums, S.off2 + na, &ctx->d_meta->n_out));
  return GIQL_OK;
}

static int plan_general(giql_hip_ctx* ctx, hipStream_t st, int n_chrom, PlanSide& A, PlanSide& B, InnerScratch& W,
                        InnerAttempt& T) {
  InnerState& S = ctx->plan.inner;
  const LinBufs& lb = W.lb;
  SortBufs& sa = *A.sort;
  SortBufs& sbb = *B.sort;
  const size_t n_small = A.n < B.n ? A.n : B.n;
  bind_status(W, B, A);
  // The join itself in B's bucket stage (bucket_sort.hip.h, FUSE == 3): one-call form, on the context's guesses (the
  // general form again, no irregular row, no row longer than the windows allow for), B the three-stage side, the A
  // rows -- fully sorted -- sparse enough for a bucket's window to stay in a block's registers.
  // (a window = the A rows within the bucket's 65536 keys + the longest rows of either side: the previous plan's
  // maxima, like the guess they validate)
  // KNOWN ODDITY (kept as it is): h_meta holds the last read-back of ANY call on the context, not of the last INNER
  // plan, so "the previous plan's maxima" may be another operator's numbers.  A candidate for a later fix with a test.
  const int wb_b = sort_local_bits(sort_tuning(ctx), B.n);
  T.general_join = T.onesweep && A.out_row && T.no_irr && ctx->plan.fuse_cap > 0 && B.n >= A.n && wb_b != 0 &&
                   T.fuse_len_ok && ctx->guess.last_span > 0 &&
                   (double)A.n * ((double)(1u << (wb_b ? wb_b : 16)) + (double)ctx->h_meta->len_max_a +
                                  (double)ctx->h_meta->len_max_b) /
                           (double)ctx->guess.last_span <= 0.5 * (double)BJ_WCAP;
  // the smaller side's chain (linearize + sort) beside the larger side's when it is small (not in the form above:
  // B's last stage reads the sorted A)
  SideChain sc(ctx, st, (T.onesweep && !T.general_join) ? n_small : 0);
  PlanSide* const sides[2] = {&A, &B};
  hipStream_t stream_of[2] = {A.n < B.n ? sc.stream() : st, A.n < B.n ? st : sc.stream()};
  const giql_side* keygen_of[2] = {nullptr, nullptr};
  if (T.keygen_g) keygen_of[T.big_side] = sides[T.big_side]->side;
  for (PlanSide* s : sides) {
    if (keygen_of[s->label]) {
      GIQL_TRY(span_digit_offsets(ctx, stream_of[s->label], lb, s->hist, s->gbase, nullptr, nullptr,
                                  "digit offsets (span histogram, general form)"));
    } else {
      GIQL_TRY(run_linearize(ctx, stream_of[s->label], *s->side, n_chrom, lb, s->which(),
                             LinTarget::keys_ends(s->sort->key[0], s->sort->end[0], s->irr_list),
                             LinOptions().counting_starts(s->starts())));
    }
  }
  if (T.onesweep) {
    GIQL_TRY(run_sort_onesweep(ctx, stream_of[0], sa,
                               A.sort_rows().keys_from(keygen_of[0], lb.abase).already_sorted(T.presorted[0])));
    FuseCount fg = {};
    if (T.general_join) {
      const FuseTarget out{A.out_row, B.out_row, ctx->plan.fuse_cap};
      // class 2: b.start in (a.start, a.end)
      fg = make_fuse_count(ctx, fuse_query(A), 1, 0xFFFFFFFFu, &out, true, B.len_max,
                           reinterpret_cast<u32*>(W.scan_chain));
    }
    GIQL_TRY(run_sort_onesweep(ctx, stream_of[1], sbb,
                               B.sort_rows().keys_from(keygen_of[1], lb.abase).fused_with(T.general_join ? &fg : nullptr)
                                   .already_sorted(T.presorted[1])));
    GIQL_TRY(sc.join());
  } else {
    GIQL_TRY(run_sort(ctx, st, sa, (u32)A.n, W.tile_hist, W.bsums));
    GIQL_TRY(run_sort(ctx, st, sbb, (u32)B.n, W.tile_hist, W.bsums));
  }
  if (T.general_join) return finish_bucket_join(ctx, st);
  // class 1 (count + the scan of its block totals) runs beside class 2 when both sides are small
  SideChain sc1(ctx, st, T.onesweep ? n_small : 0);
  hipStream_t st1 = sc1.stream();
  GIQL_TRY(run_class_counts(ctx, S, W, sa, sbb, A.n, B.n, A.irr, B.irr, st1, st));
  GIQL_TRY(sc1.join());
  GIQL_TRY(read_meta(ctx, st));
  ctx->plan.n_c1 = ctx->h_meta->n_out_c1;
  ctx->plan.n_reg = ctx->h_meta->n_out + ctx->plan.n_c1;
  return GIQL_OK;
}

// After the attempt's final read-back: the ONLY place that decides whether a guess missed, and (bar last_span's early
// write in begin_attempt) that writes the INNER guesses.  false: a guess missed -- the result is not valid, the
// guesses are dropped, and the plan is repeated from the numbers just read.
static bool settle_guesses(giql_hip_ctx* ctx, const InnerAttempt& T, size_t na, size_t nb) {
  const DevMeta& m = *ctx->h_meta;
  Guesses& g = ctx->guess;
  const bool any_irr = m.irr_a + m.irr_b > 0;
  if (T.onesweep) {
    int form;
    i64 len;
    decide_form(m, na, nb, ctx->sw.no_uniform, form, len);
    const bool aligned_now = m.aligned_ok != 0;
    const bool fuse_len_ok_now = fuse_len_ok(m, form);  // (the query side of the form just decided)
    // the lengths say another form, or another fixed length
    const bool form_wrong = form != T.form || len != T.uni_len;
    // the span pass counted digits of aligned keys, and the data does not take the aligned layout
    const bool layout_wrong = T.want_hist && !aligned_now;
    // a query side sorted without its low digits must hold no irregular row (their sentinel keys must come last)
    const bool coarse_wrong = T.q_skip != 0 && any_irr;
    // a side sorted from its raw columns must hold no irregular row (its length range starts above 0); such a row
    // was keyed as if regular, and never listed
    const bool keygen_wrong = (T.keygen_g && len_min_of(m, T.big_side) <= 0) ||
                              (T.keygen_q && len_min_of(m, 1 - T.big_side) <= 0);
    // the fused count's windows allow for rows up to BS_FUSE_WCAP long
    const bool fuse_wrong = T.count_fused() && !fuse_len_ok_now;
    // a side taken as sorted must be: an out-of-order row was left where it was
    const bool sorted_wrong = (T.presorted[0] && m.unsorted_a != 0) || (T.presorted[1] && m.unsorted_b != 0);
    // a join in the bucket stage that did not stand (the pairs did not fit the caller's buffers, or a guess failed)
    // left no plan arrays for the ordinary fill: plan again, unspeculated -- which never takes that form
    const bool join_wrong = T.bucket_join() && !ctx->plan.fuse_done;
    // (these three are stored before a missed guess returns)
    if (keygen_wrong) g.last_no_irr = false;
    g.spec_fuse_len_ok = fuse_len_ok_now;
    g.spec_sorted[0] = m.unsorted_a == 0;
    g.spec_sorted[1] = m.unsorted_b == 0;
    if (T.speculated && (form_wrong || layout_wrong || coarse_wrong || keygen_wrong || fuse_wrong || sorted_wrong ||
                         join_wrong)) {
      g.spec_valid = false;  // wrong guess: plan again from the numbers just read
      g.spec_misses++;
      ctx->plan.fuse_done = false;
      return false;
    }
    g.spec_valid = true;
    g.spec_form = form;
    g.spec_len = len;
    // the layout is probed only when the span histogram ran; a plan that skipped it for a
    // form mismatch leaves the last answer (a later form change re-plans unspeculated anyway)
    if (T.want_hist) g.spec_aligned = aligned_now;
  }
  g.last_span = m.total_span;
  g.last_no_irr = !any_irr;
  return true;
}

// The pairs of irregular rows (canonical end <= start), counted per row of either side against the other's list.
static int plan_irregular(giql_hip_ctx* ctx, hipStream_t st, const PlanSide& A, const PlanSide& B, InnerScratch& W) {
  const size_t nq = A.n + B.n;
  {
    Phase ph(ctx, st, GIQL_PH_IRREGULAR);
    hipLaunchKernelGGL(k_irr_count, dim3(cdiv(nq, 256)), dim3(256), 0, st, view_of(*A.side), view_of(*B.side),
                       A.irr_list, B.irr_list, ctx->d_meta, W.irr_cnt);
    GIQL_TRY(post_launch("irregular count"));
  }
  GIQL_TRY(run_scan<u64>(ctx, st, GIQL_PH_IRREGULAR, W.irr_cnt, nq, ctx->plan.irr_off, W.bsums,
                         ctx->plan.irr_off + nq));
  HIP_TRY(hipMemcpyAsync(&ctx->d_meta->n_out_irr, ctx->plan.irr_off + nq, sizeof(u64),
                         hipMemcpyDeviceToDevice, st));
  GIQL_TRY(read_meta(ctx, st));
  ctx->plan.n_irr = ctx->h_meta->n_out_irr;
  return GIQL_OK;
}

// One attempt at a plan, in the plan's labels (A = the smaller side when giql_hip_inner_plan_dev_impl exchanged them:
// ctx->plan.swapped).
static int inner_plan_core(giql_hip_ctx* ctx, const giql_side* a, const giql_side* b,
                           int32_t n_chrom, void* stream, int64_t* n_pairs) {
  hipStream_t st = (hipStream_t)stream;
  ctx->plan.fuse_done = false;
  ctx->stats.n_a = a->n;  // (in the plan's labels: giql_hip_inner_plan_dev_impl labels them back)
  ctx->stats.n_b = b->n;
  ctx->plan.side_a = *a;
  ctx->plan.side_b = *b;
  ctx->plan.n_a = (u32)a->n;
  ctx->plan.n_b = (u32)b->n;
  ctx->plan.n_chrom = n_chrom;
  ctx->plan.n_reg = ctx->plan.n_irr = ctx->plan.n_c1 = 0;
  ctx->plan.widen = -1;
  *n_pairs = 0;
  if (a->n == 0 || b->n == 0 || n_chrom == 0) {  // empty result (tests :4173-4229)
    ctx->kept = Plan::INNER;
    ctx->plan.plan_is_join = false;
    return GIQL_OK;
  }
  const size_t na = (size_t)a->n, nb = (size_t)b->n;

  // ---- carve the arena (dry run for the size, then for real)
  InnerState& S = ctx->plan.inner;
  InnerScratch W;
  InnerAttempt T;
  T.onesweep = !ctx->sw.classic_sort && na <= OS_MAX_ROWS && nb <= OS_MAX_ROWS;
  T.big_side = nb >= na ? 1 : 0;
  S.c1_items = nb <= C1_SMALL_ROWS ? 2 : C1_ITEMS_MAX;
  S.nt1 = cdiv(nb, (u32)(C1_NT * S.c1_items));
  S.c1_fill = nb <= C1_SMALL_ROWS;
  S.nt2 = cdiv(na, RC_NT * RC_ITEMS_C2);
  GIQL_TRY(claim_arena(ctx, st, [&](char* base) { return carve_inner(ctx, base, na, nb, n_chrom, T.onesweep, W); }));
  // ---- the two sides.  The caller's output rows follow the sides HERE, for this attempt only: plan.fuse_a / fuse_b
  // stay in the caller's labels, so an attempt that with_order_fallback repeats binds them afresh.
  PlanSide A, B;
  A.side = a, B.side = b;
  A.n = na, B.n = nb;
  A.label = 0, B.label = 1;
  A.sort = &S.sa, B.sort = &S.sb;
  A.hist = W.hist[0], B.hist = W.hist[1];
  A.gbase = W.gbase[0], B.gbase = W.gbase[1];
  A.irr_list = ctx->plan.irr_a_list, B.irr_list = ctx->plan.irr_b_list;
  A.irr = &ctx->d_meta->irr_a, B.irr = &ctx->d_meta->irr_b;
  A.len_max = &ctx->d_meta->len_max_a, B.len_max = &ctx->d_meta->len_max_b;
  A.out_row = ctx->plan.swapped ? ctx->plan.fuse_b : ctx->plan.fuse_a;
  B.out_row = ctx->plan.swapped ? ctx->plan.fuse_a : ctx->plan.fuse_b;

  ZeroedScope zeroed_scope{ctx};  // the helpers skip their own memsets on what zero_inner_scratch zeroes
  UnstableFirstPass unstable_first{ctx};  // an INNER join needs no order among rows of equal keys: first passes rank by LDS atomics
  if (T.onesweep) GIQL_TRY(zero_inner_scratch(ctx, st, W, na > nb ? na : nb));

  GIQL_TRY(begin_attempt(ctx, st, A, B, n_chrom, W, T));
  S.uniform = T.form;
  ctx->call.used_sorted[0] = T.presorted[0];
  ctx->call.used_sorted[1] = T.presorted[1];
  if (T.form == 1) {
    GIQL_TRY(plan_uniform(ctx, st, n_chrom, /*Q=*/A, /*U=*/B, W, T));
  } else if (T.form == 2) {
    GIQL_TRY(plan_uniform(ctx, st, n_chrom, /*Q=*/B, /*U=*/A, W, T));
  } else {
    GIQL_TRY(plan_general(ctx, st, n_chrom, A, B, W, T));
  }
  if (!settle_guesses(ctx, T, na, nb)) return GIQL_STATUS_GUESS_MISSED;
  ctx->stats.n_irregular_a = ctx->h_meta->irr_a;
  ctx->stats.n_irregular_b = ctx->h_meta->irr_b;
  ctx->stats.span = (int64_t)ctx->h_meta->total_span;

  if (ctx->h_meta->irr_a + ctx->h_meta->irr_b > 0) GIQL_TRY(plan_irregular(ctx, st, A, B, W));
  collect_spans(ctx);
  // which form ran: 0 general, 1 B uniform, 2 A uniform; bit 4: the fixed-length side was sorted
  // from its raw columns (histogram in the span pass, no linearize pass)
  ctx->stats.reserved = S.uniform | ((T.keygen_u || T.keygen_g) ? 0x10 : 0);
  ctx->stats.n_out = (int64_t)(ctx->plan.n_reg + ctx->plan.n_irr);
  *n_pairs = (int64_t)(ctx->plan.n_reg + ctx->plan.n_irr);
  ctx->kept = Plan::INNER;
  ctx->plan.plan_is_join = T.bucket_join();
  return GIQL_OK;
}

// The plan works with "B = the larger side": the general form keeps per-row arrays (bounds, counts, 64-bit
// offsets) for its class-2 queries, the A rows, and only block totals for class 1, the B rows, so the
// sides' roles are not symmetric in cost (10M x 100M reads: 4.4 ms; the same tables as (100M, 10M):
// 12.9 ms before this swap).  INTERSECTS is symmetric, so a call with the larger table first is planned
// with the sides exchanged and everything that leaves the context (pairs, stats, the exported plan) is
// labelled back; only the order of the pairs -- never part of the contract -- differs.  (The offered output
// buffers follow the sides where inner_plan_core binds them.)
static int giql_hip_inner_plan_dev_impl(giql_hip_ctx* ctx, const giql_side* a, const giql_side* b,
                                        int32_t n_chrom, void* stream, int64_t* n_pairs) {
  if (!ctx || !n_pairs) return set_err(GIQL_ERR_INVALID, "ctx/n_pairs is NULL");
  GIQL_TRY(begin_pair_call(ctx, a, b, n_chrom));
  const bool swap = a->n > b->n;
  ctx->plan.swapped = swap;
  if (!swap) return inner_plan_core(ctx, a, b, n_chrom, stream, n_pairs);
  const int rc = inner_plan_core(ctx, b, a, n_chrom, stream, n_pairs);
  // stats in the caller's labels
  giql_hip_stats& stt = ctx->stats;
  const int64_t tn = stt.n_a;
  stt.n_a = stt.n_b;
  stt.n_b = tn;
  const int64_t ti = stt.n_irregular_a;
  stt.n_irregular_a = stt.n_irregular_b;
  stt.n_irregular_b = ti;
  const int form = stt.reserved & 0xF;
  if (form == 1 || form == 2) stt.reserved = (stt.reserved & ~0xF) | (3 - form);
  return rc;
}

int giql_hip_inner_plan_dev(giql_hip_ctx* ctx, const giql_side* a, const giql_side* b, int32_t n_chrom,
                            void* stream, int64_t* n_pairs) {
  return with_order_fallback(ctx, [&] { return giql_hip_inner_plan_dev_impl(ctx, a, b, n_chrom, stream, n_pairs); });
}

int giql_hip_inner_fill_dev(giql_hip_ctx* ctx, int32_t* row_a, int32_t* row_b, int64_t capacity,
                            void* stream) {
  if (!ctx) return set_err(GIQL_ERR_INVALID, "ctx is NULL");
  if (ctx->kept != Plan::INNER) return set_err(GIQL_ERR_STATE, "inner_fill without a successful inner_plan");
  const u64 total = ctx->plan.n_reg + ctx->plan.n_irr;
  if (total == 0) return GIQL_OK;
  if (ctx->plan.plan_is_join)
    return set_err(GIQL_ERR_STATE, "the last giql_hip_inner_join_dev wrote its pairs itself and kept no plan: "
                                   "call giql_hip_inner_plan_dev first");
  if (!row_a || !row_b) return set_err(GIQL_ERR_INVALID, "row_a/row_b is NULL");
  if (capacity < 0 || (u64)capacity < total)
    return set_err(GIQL_ERR_CAPACITY, "capacity %lld < %llu pairs", (long long)capacity,
                   (unsigned long long)total);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  if (ctx->plan.swapped) {  // planned with the sides exchanged: the plan's "A" rows are the caller's B rows
    int32_t* t = row_a;
    row_a = row_b;
    row_b = t;
  }
  const u32 nq = ctx->plan.n_a + ctx->plan.n_b;
  InnerState& S = ctx->plan.inner;
  const u32* irr_a = &ctx->d_meta->irr_a;
  const u32* irr_b = &ctx->d_meta->irr_b;
  const u64 p1 = ctx->plan.n_c1, p2 = ctx->plan.n_reg - ctx->plan.n_c1;
  // who plays "query" in the range-fill: A rows (general class 2, or B uniform),
  // or B rows (A uniform) -- bound once, like the plan's PlanSides
  struct FillSide {
    const u32* rid;
    u32 n;
    int32_t* row;
  };
  const FillSide fa{S.sa.rid[0], ctx->plan.n_a, row_a}, fb{S.sb.rid[0], ctx->plan.n_b, row_b};
  const FillSide& Q = S.uniform != 2 ? fa : fb;
  const FillSide& U = S.uniform != 2 ? fb : fa;
  u32 nt2 = 0, nt1f = 0;
  const bool c1_fill = S.uniform == 0 && S.c1_fill && p1 > 0;
  if (p2 > 0 || c1_fill) {
    constexpr u32 T2 = FILL_NT * FILL_ITEMS_C2;
    const u64 nt2_64 = (p2 + T2 - 1) / T2, nt1_64 = c1_fill ? (p1 + T2 - 1) / T2 : 0;
    if (nt2_64 + nt1_64 > 0x7FFFFFF0ull) return set_err(GIQL_ERR_INVALID, "output too large");
    nt2 = (u32)nt2_64;
    nt1f = (u32)nt1_64;
    const size_t part_need = (size_t)nt2 + 2 + (c1_fill ? (size_t)nt1f + 2 : 0);
    GIQL_TRY(grow_part(ctx, part_need, st));
    Phase ph(ctx, st, GIQL_PH_PARTITION);
    if (p2 > 0)
      hipLaunchKernelGGL(k_partition, dim3(cdiv((u64)nt2 + 1, 256)), dim3(256), 0, st, S.off2, Q.n,
                         (u64)0, T2, nt2, ctx->part);
    if (c1_fill)  // class 1's tiles behind class 2's in the partition array
      hipLaunchKernelGGL(k_partition, dim3(cdiv((u64)nt1f + 1, 256)), dim3(256), 0, st, S.off1, ctx->plan.n_b,
                         (u64)0, T2, nt1f, ctx->part + nt2 + 2);
  }
  {
    Phase ph(ctx, st, GIQL_PH_FILL, 2);
    // class 1 -> outputs [0, p1): query = B row, matches = A rows
    if (c1_fill)
      hipLaunchKernelGGL((k_fill<FILL_ITEMS_C2>), dim3(nt1f), dim3(FILL_NT), 0, st, S.off1, S.lo1, S.sb.rid[0],
                         ctx->plan.n_b, S.sa.rid[0], ctx->part + nt2 + 2, (u64)0, p1, row_b, row_a);
    else if (p1 > 0 && S.c1_items == 2)
      hipLaunchKernelGGL(k_c1_emit<2>, dim3(S.nt1), dim3(C1_NT), 0, st, S.sb.key[0], S.sb.end[0],
                         S.sb.rid[0], ctx->plan.n_b, irr_b, S.sa.key[0], S.sa.rid[0], ctx->plan.n_a, irr_a,
                         S.wlo1, S.c1_base, (u64)0, row_b, row_a);
    else if (p1 > 0)
      hipLaunchKernelGGL(k_c1_emit<C1_ITEMS_MAX>, dim3(S.nt1), dim3(C1_NT), 0, st, S.sb.key[0], S.sb.end[0],
                         S.sb.rid[0], ctx->plan.n_b, irr_b, S.sa.key[0], S.sa.rid[0], ctx->plan.n_a, irr_a,
                         S.wlo1, S.c1_base, (u64)0, row_b, row_a);
    // range fill -> outputs [p1, p1 + p2)
    if (p2 > 0)
      hipLaunchKernelGGL((k_fill<FILL_ITEMS_C2>), dim3(nt2), dim3(FILL_NT), 0, st, S.off2, S.lo2, Q.rid,
                         Q.n, U.rid, ctx->part, (u64)0, p2, Q.row + p1, U.row + p1);
    GIQL_TRY(post_launch("fill"));
  }
  if (ctx->plan.n_irr > 0) {
    Phase ph(ctx, st, GIQL_PH_IRREGULAR);
    if (ctx->plan.widen >= 0)
      hipLaunchKernelGGL(k_window_irr_fill, dim3(cdiv(nq, 256)), dim3(256), 0, st, view_of(ctx->plan.side_a),
                         view_of(ctx->plan.side_b), ctx->plan.irr_a_list, ctx->plan.irr_b_list, ctx->d_meta,
                         ctx->plan.widen, ctx->plan.irr_off, row_a + ctx->plan.n_reg, row_b + ctx->plan.n_reg);
    else
      hipLaunchKernelGGL(k_irr_fill, dim3(cdiv(nq, 256)), dim3(256), 0, st, view_of(ctx->plan.side_a),
                         view_of(ctx->plan.side_b), ctx->plan.irr_a_list, ctx->plan.irr_b_list, ctx->d_meta,
                         ctx->plan.irr_off, row_a + ctx->plan.n_reg, row_b + ctx->plan.n_reg);
    GIQL_TRY(post_launch("irregular fill"));
  }
  return GIQL_OK;
}

// Plan + fill in one call into caller-owned buffers.  When the context's guesses hold (same
// join form as its previous plan, no irregular rows, the pairs fit `capacity`) the fill has
// already been launched inside the plan, with no stream sync between the two; otherwise the
// ordinary fill runs here.  GIQL_ERR_CAPACITY leaves the plan valid: *n_pairs tells the
// size to offer to giql_hip_inner_fill_dev.
int giql_hip_inner_join_dev(giql_hip_ctx* ctx, const giql_side* a, const giql_side* b, int32_t n_chrom,
                            int32_t* row_a, int32_t* row_b, int64_t capacity, void* stream,
                            int64_t* n_pairs) {
  if (!ctx || !n_pairs) return set_err(GIQL_ERR_INVALID, "ctx/n_pairs is NULL");
  if (capacity < 0 || (capacity > 0 && (!row_a || !row_b)))
    return set_err(GIQL_ERR_INVALID, "bad output buffers");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  {  // the merge-path partition array must exist before the plan can launch the fill
    constexpr u32 T2 = FILL_NT * FILL_ITEMS_C2;
    const u64 nt_cap = ((u64)capacity + T2 - 1) / T2;
    if (nt_cap <= 0x7FFFFFF0ull) GIQL_TRY(grow_part(ctx, (size_t)nt_cap + 2, st));
  }
  ctx->plan.fuse_a = row_a;
  ctx->plan.fuse_b = row_b;
  ctx->plan.fuse_cap = (u64)capacity;
  const int rc = giql_hip_inner_plan_dev(ctx, a, b, n_chrom, stream, n_pairs);
  ctx->plan.fuse_a = ctx->plan.fuse_b = nullptr;
  ctx->plan.fuse_cap = 0;
  if (rc != GIQL_OK) return rc;
  if (ctx->plan.fuse_done) return GIQL_OK;
  if (*n_pairs > capacity)
    return set_err(GIQL_ERR_CAPACITY, "capacity %lld < %lld pairs", (long long)capacity, (long long)*n_pairs);
  return giql_hip_inner_fill_dev(ctx, row_a, row_b, capacity, stream);
}

// ------------------------------------------------- within-distance join / DISTANCE
// DISTANCE needs start <= end on every row of both sides; which side does not: for callers in giql_hip_stats
// (n_irregular_a / n_irregular_b = -1), not only in the message.
static int reject_inverted(giql_hip_ctx* ctx) {
  if (!ctx->h_meta->inverted_a && !ctx->h_meta->inverted_b) return GIQL_OK;
  if (ctx->h_meta->inverted_a) ctx->stats.n_irregular_a = -1;
  if (ctx->h_meta->inverted_b) ctx->stats.n_irregular_b = -1;
  return set_err(GIQL_ERR_INVALID, "DISTANCE: side %s has a row with start > end", ctx->h_meta->inverted_a ? "a" : "b");
}

// coordinates of one chromosome are less than 2^32 + 2 apart: a larger N selects the same pairs, and the sums of the
// widened rows stay far from the ends of int64
static inline i64 clamp_widen(int64_t max_distance) {
  return max_distance > ((i64)1 << 33) ? ((i64)1 << 33) : (i64)max_distance;
}

// A widened by `widen` on both ends and keyed on the axis run_spans(pad = 1) laid out over the sides a and b, its
// ends clamped to that padding; with the digit histogram and bases of its sort.  irr_list: rows left zero-length get
// the sentinel key and a place in the list (k_window_linearize); nullptr: every row keeps its key (k_rp_window_keys).
static int key_widened_side(giql_hip_ctx* ctx, hipStream_t st, const giql_side& a, const giql_side& b, int n_chrom,
                            const LinBufs& lb, i64 widen, SortBufs& sa, u32* irr_list, u32* hist, u32* gbase) {
  int lo_pad, hi_pad;
  window_pads(a, b, /*pad=*/1, lo_pad, hi_pad);
  HIP_TRY(hipMemsetAsync(hist, 0, (size_t)LIN_HIST_REPLICAS * 1024 * sizeof(u32), st));
  Phase ph(ctx, st, GIQL_PH_LINEARIZE, 2);
  u32 grid = cdiv((u64)a.n, LIN_NT);
  if (grid > (u32)LIN_MAX_BLOCKS) grid = LIN_MAX_BLOCKS;
  if (irr_list)
    hipLaunchKernelGGL(k_window_linearize, dim3(grid), dim3(LIN_NT), 0, st, a.chrom, a.start, a.end, (u32)a.n,
                       a.start_off, a.end_off, n_chrom, lb.chrom_base, lb.gmin, lb.gmax, lo_pad, hi_pad, widen,
                       sa.key[0], sa.end[0], irr_list, ctx->d_meta, hist);
  else
    hipLaunchKernelGGL(k_rp_window_keys, dim3(grid), dim3(LIN_NT), 0, st, a.chrom, a.start, a.end, (u32)a.n,
                       a.start_off, a.end_off, n_chrom, lb.chrom_base, lb.gmin, lb.gmax, lo_pad, hi_pad, widen,
                       sa.key[0], sa.end[0], ctx->d_meta, hist);
  hipLaunchKernelGGL(k_digit_offsets, dim3(4), dim3(256), 0, st, hist, (u32)LIN_HIST_REPLICAS, gbase);
  return post_launch(irr_list ? "window linearize" : "row predicate window keys");
}

// giql_hip_window_plan_dev: the pairs with DISTANCE(a, b) <= max_distance, as an INNER plan that giql_hip_inner_fill_dev
// fills (distance_kernels.hip.h has the equivalence and the clamp).  ONE form is routed, the general two-class one, in
// its plainest shape: span pass padded by one position per chromosome end -> ONE read-back (chrom ids, the 32-bit
// axis, inverted rows) -> A widened and keyed by k_window_linearize, B by k_linearize -> both sorted -> the class-1 and
// class-2 range counts and scans of plan_general -> the widened literal kernels for zero-length rows.  Nothing is
// speculated and no INNER guess is read or written: the uniform-length form, the sorts from raw columns, the fused
// count and the bucket-stage join are not reachable with a widening, and a plain INTERSECTS plan after this one
// finds its guesses as it left them.
static int giql_hip_window_plan_dev_impl(giql_hip_ctx* ctx, const giql_side* a, const giql_side* b, int32_t n_chrom,
                                         int64_t max_distance, void* stream, int64_t* n_pairs) {
  if (!ctx || !n_pairs) return set_err(GIQL_ERR_INVALID, "ctx/n_pairs is NULL");
  if (max_distance < 0) return set_err(GIQL_ERR_INVALID, "max_distance < 0");
  GIQL_TRY(begin_pair_call(ctx, a, b, n_chrom));
  hipStream_t st = (hipStream_t)stream;
  InnerPlan& P = ctx->plan;
  P.swapped = false;
  P.plan_is_join = false;
  P.fuse_done = false;
  P.side_a = *a;
  P.side_b = *b;
  P.n_a = (u32)a->n;
  P.n_b = (u32)b->n;
  P.n_chrom = n_chrom;
  P.n_reg = P.n_irr = P.n_c1 = 0;
  P.widen = -1;
  *n_pairs = 0;
  if (a->n == 0 || b->n == 0 || n_chrom == 0) {  // empty result, as the INNER plan's
    ctx->kept = Plan::INNER;
    return GIQL_OK;
  }
  const size_t na = (size_t)a->n, nb = (size_t)b->n, nq = na + nb;
  GIQL_TRY(check_rows_fit(na, nb));
  const i64 widen = clamp_widen(max_distance);
  InnerState& S = P.inner;
  InnerScratch W;
  constexpr u32 TQ2 = RC_NT * RC_ITEMS_C2;
  S.uniform = 0;
  S.c1_items = nb <= C1_SMALL_ROWS ? 2 : C1_ITEMS_MAX;
  S.nt1 = cdiv(nb, (u32)(C1_NT * S.c1_items));
  S.c1_fill = nb <= C1_SMALL_ROWS;
  S.nt2 = cdiv(na, TQ2);
  GIQL_TRY(claim_arena(ctx, st, [&](char* base) { return carve_inner(ctx, base, na, nb, n_chrom, true, W); }));
  GIQL_TRY(run_spans(ctx, st, *a, *b, n_chrom, W.lb, -1, nullptr, /*pad=*/1));
  GIQL_TRY(read_meta(ctx, st));
  GIQL_TRY(reject_inverted(ctx));
  ctx->guess.last_span = ctx->h_meta->total_span;  // known before anything is sorted: the sort form follows the real density
  SortBufs& sa = S.sa;
  SortBufs& sbb = S.sb;
  u32* const status_a = na <= nb ? W.os_status2 : W.os_status;
  u32* const status_b = na <= nb ? W.os_status : W.os_status2;
  GIQL_TRY(key_widened_side(ctx, st, *a, *b, n_chrom, W.lb, widen, sa, P.irr_a_list, W.hist[0], W.gbase[0]));
  GIQL_TRY(run_linearize(ctx, st, *b, n_chrom, W.lb, Side::B, LinTarget::keys_ends(sbb.key[0], sbb.end[0], P.irr_b_list),
                         LinOptions().counting_starts({W.hist[1], W.gbase[1]})));
  GIQL_TRY(run_sort_onesweep(ctx, st, sa, SortRequest::rows((u32)na, W.gbase[0], status_a)));
  GIQL_TRY(run_sort_onesweep(ctx, st, sbb, SortRequest::rows((u32)nb, W.gbase[1], status_b)));
  const u32* irr_a = &ctx->d_meta->irr_a;
  const u32* irr_b = &ctx->d_meta->irr_b;
  // the counts and scans of plan_general, over the widened A (class 1 and class 2 on the one stream)
  GIQL_TRY(run_class_counts(ctx, S, W, sa, sbb, na, nb, irr_a, irr_b, st, st));
  GIQL_TRY(read_meta(ctx, st));
  P.n_c1 = ctx->h_meta->n_out_c1;
  P.n_reg = ctx->h_meta->n_out + P.n_c1;
  ctx->stats.n_irregular_a = ctx->h_meta->irr_a;
  ctx->stats.n_irregular_b = ctx->h_meta->irr_b;
  ctx->stats.span = (int64_t)ctx->h_meta->total_span;
  if (ctx->h_meta->irr_a + ctx->h_meta->irr_b > 0) {
    {
      Phase ph(ctx, st, GIQL_PH_IRREGULAR);
      hipLaunchKernelGGL(k_window_irr_count, dim3(cdiv(nq, 256)), dim3(256), 0, st, view_of(*a), view_of(*b),
                         P.irr_a_list, P.irr_b_list, ctx->d_meta, widen, W.irr_cnt);
      GIQL_TRY(post_launch("window irregular count"));
    }
    GIQL_TRY(run_scan<u64>(ctx, st, GIQL_PH_IRREGULAR, W.irr_cnt, nq, P.irr_off, W.bsums, P.irr_off + nq,
                           &ctx->d_meta->n_out_irr));
    GIQL_TRY(read_meta(ctx, st));
    P.n_irr = ctx->h_meta->n_out_irr;
  }
  collect_spans(ctx);
  ctx->stats.reserved = 0;  // join_form: the general two-class form, the only one a widening reaches
  ctx->stats.n_out = (int64_t)(P.n_reg + P.n_irr);
  *n_pairs = (int64_t)(P.n_reg + P.n_irr);
  P.widen = widen;
  ctx->kept = Plan::INNER;
  return GIQL_OK;
}

int giql_hip_window_plan_dev(giql_hip_ctx* ctx, const giql_side* a, const giql_side* b, int32_t n_chrom,
                             int64_t max_distance, void* stream, int64_t* n_pairs) {
  return with_order_fallback(
      ctx, [&] { return giql_hip_window_plan_dev_impl(ctx, a, b, n_chrom, max_distance, stream, n_pairs); });
}

// DISTANCE(a[row_a[i]], b[row_b[i]]) per pair (k_pair_distance).  No workspace: begin_call_beside_plan.
int giql_hip_distance_dev(giql_hip_ctx* ctx, const giql_side* a, const giql_side* b, const int32_t* row_a,
                          const int32_t* row_b, int64_t n, const int32_t* strand_a, const int32_t* strand_b,
                          int32_t flags, int64_t* dist_out, uint8_t* valid_out, void* stream) {
  if (!ctx) return set_err(GIQL_ERR_INVALID, "ctx is NULL");
  GIQL_TRY(check_side(a, "a"));
  GIQL_TRY(check_side(b, "b"));
  if (n < 0) return set_err(GIQL_ERR_INVALID, "n < 0");
  if (flags & ~3) return set_err(GIQL_ERR_INVALID, "flags outside {1 = signed, 2 = stranded}");
  if (n > 0 && (!row_a || !row_b || !dist_out || !valid_out))
    return set_err(GIQL_ERR_INVALID, "row_a/row_b/dist_out/valid_out is NULL");
  if ((flags & 2) && ((a->n > 0 && !strand_a) || (b->n > 0 && !strand_b)))
    return set_err(GIQL_ERR_INVALID, "stranded DISTANCE without strand codes");
  if (n == 0) return GIQL_OK;
  GIQL_TRY(begin_call_beside_plan(ctx, a->n, b->n));
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(&ctx->d_meta->status, 0, sizeof(int), st));
  u32 grid = cdiv((u64)n, DIST_NT * 4);
  if (grid > GIQL_STREAM_GRID) grid = GIQL_STREAM_GRID;
  {
    Phase ph(ctx, st, GIQL_PH_AUX);
    ctx->stats.phase_bytes[GIQL_PH_AUX] += (int64_t)33 * n;  // 8 B of ids, four 4 B coordinate gathers, 9 B written
    hipLaunchKernelGGL(k_pair_distance, dim3(grid), dim3(DIST_NT), 0, st, view_of(*a), view_of(*b), row_a, row_b, (u64)n,
                       strand_a, strand_b, (u32)flags, dist_out, valid_out, ctx->d_meta);
    GIQL_TRY(post_launch("pair distance"));
  }
  if (read_meta(ctx, st) != GIQL_OK) {
    if (ctx->h_meta->status == GIQL_ERR_INVALID) return set_err(GIQL_ERR_INVALID, "a row id is outside its table");
    return ctx->h_meta->status ? ctx->h_meta->status : GIQL_ERR_HIP;
  }
  collect_spans(ctx);
  ctx->stats.n_out = n;
  return GIQL_OK;
}

// ------------------------------------------------------------- table index
// The reference tells its users to CREATE INDEX ... (chrom, start, "end") on both join sides
// (docs/transpilation/performance.rst:111-130): what the engine keeps between queries.  Here: the properties of a
// TABLE that every join over it recomputes -- span and chromosome bases, the fixed length, the (key, rid) rows
// grouped by 65,536-key bucket and sorted -- kept in HBM as an explicit object.  A join against an index
// (giql_hip_inner_join_indexed_dev) is the other side's span pass + sort + the bucket stage: the larger table's
// span pass (1.2 GB read at 100M rows) and its two global sort passes (3.2 GB) are not repeated.  An extra, never
// the headline: bench.py times it as its own workload beside the build time of the index.
struct giql_hip_index {
  int device = 0;
  u32 n = 0;
  int n_chrom = 0;
  bool general = false;    // rows of any length: (key, end, rid); else fixed length: (key, rid)
  i64 uni_len = 0;         // the fixed canonical length (0 in the general form)
  int len_max = 0;         // the longest row
  u64 span = 0;
  u32 sentinel = 0;        // one past the largest key of the axis
  int wbits = 16;          // key bits of a bucket (16; 15 / 14 / 13 for tables past ~2,800 rows per 65,536 positions)
  DevArray<u32> key, end, rid;  // [n] sorted by key (every bucket sorted in place)
  DevArray<u32> small;     // the sort's digit offsets gbase[4][256] | first[n_chrom + 1]: chromosome c owns keys [first[c], first[c + 1])
  // what the per-row operators read (giql_hip_index_prepare_rows_dev: built on their first call, never at creation)
  bool rows_ready = false;
  DevArray<u32> bnd_key;      // [2^(32 - wbits) + 1] directory over key: first row with key >= v << wbits
  DevArray<u32> end_sorted;   // general form: [n] the end keys alone, sorted ...
  DevArray<u32> bnd_end;      // ... and their directory
  // what NEAREST reads (giql_hip_index_prepare_nearest_dev: on its first call, never at creation) beside bnd_key,
  // which either preparation builds and the other finds here
  int nearest_state = 0;      // 0: not prepared; 1: ready; -1: the table does not take the NEAREST form (remembered)
  DevArray<u32> chrom_lo;     // [n_chrom + 1] rank of first[c] among the keys
  DevArray<u32> nr_rid;       // general form: [n] the row ids in (start, end) order ...
  DevArray<u32> nr_pmax;      // ... and the prefix max of the end keys in that order
  // what giql_hip_index_info reports: the arrays the index owns at this moment (a preparation moves its arrays in as
  // its last step, so one that declined or failed has added nothing)
  size_t bytes() const {
    size_t sum = 0;
    for (const DevArray<u32>* b : {&key, &end, &rid, &small, &bnd_key, &end_sorted, &bnd_end, &chrom_lo, &nr_rid, &nr_pmax})
      sum += b->bytes();
    return sum;
  }
};

int giql_hip_index_destroy(giql_hip_index* idx) {
  if (!idx) return GIQL_OK;
  (void)hipSetDevice(idx->device);
  delete idx;
  return GIQL_OK;
}

int giql_hip_index_info(const giql_hip_index* idx, int64_t* n_rows, int64_t* bytes, int32_t* general, int64_t* span) {
  if (!idx) return set_err(GIQL_ERR_INVALID, "index is NULL");
  if (n_rows) *n_rows = idx->n;
  if (bytes) *bytes = (int64_t)idx->bytes();
  if (general) *general = idx->general ? 1 : 0;
  if (span) *span = (int64_t)idx->span;
  return GIQL_OK;
}

int giql_hip_index_create_dev(giql_hip_ctx* ctx, const giql_side* side, int32_t n_chrom, void* stream,
                              giql_hip_index** out) {
  if (!ctx || !out) return set_err(GIQL_ERR_INVALID, "ctx/out is NULL");
  *out = nullptr;
  GIQL_TRY(check_side(side, "side"));
  if (n_chrom < 1 || n_chrom > MM_HIST_CHROMS)
    return set_err(GIQL_ERR_STATE, "a table index takes 1..%d chromosomes (the 2^24-aligned axis), got %d", MM_HIST_CHROMS, n_chrom);
  if (side->n < 1 || (size_t)side->n > OS_MAX_ROWS) return set_err(GIQL_ERR_STATE, "a table index takes 1..2^30-1 rows");
  if (ctx->sw.classic_sort || ctx->sw.os_variant != 0 || !ctx->bucket_bnd)
    return set_err(GIQL_ERR_STATE, "this context cannot run the three-stage sort (GIQL_HIP_SORT / GIQL_HIP_OS_VARIANT)");
  GIQL_TRY(begin_call(ctx));
  hipStream_t st = (hipStream_t)stream;
  const size_t n = (size_t)side->n;
  LinBufs lb;
  SortBufs scratch;  // buffer 1 of the sort (buffer 0 = the index's own arrays)
  u32 *hist = nullptr, *gbase = nullptr, *status = nullptr;
  ZeroSpan zero;
  auto carve = [&](char* base) {
    Carver c{base};
    common_sizes(c, n_chrom, lb);
    scratch.key[1] = c.take<u32>(n);
    scratch.end[1] = c.take<u32>(n);
    scratch.rid[1] = c.take<u32>(n);
    c.open_zeroed();
    hist = c.take<u32>((size_t)LIN_HIST_REPLICAS * 1024);
    lb.top_partial = c.take<u32>((size_t)LIN_HIST_REPLICAS * MM_TOP_WORDS);
    gbase = c.take<u32>(1024);
    lb.abase = c.take<u32>(MM_HIST_CHROMS);
    status = c.take<u32>(3 * os_pass_words(n));
    zero = c.close_zeroed();
    return c.off;
  };
  GIQL_TRY(claim_arena(ctx, st, carve));
  std::unique_ptr<giql_hip_index> idx(new (std::nothrow) giql_hip_index());  // released on every early way out
  if (!idx) return set_err(GIQL_ERR_NOMEM, "out of host memory");
  ZeroedScope zeroed_scope{ctx};
  idx->device = ctx->device;
  idx->n = (u32)n;
  idx->n_chrom = n_chrom;
  GIQL_TRY(zero_span(ctx, st, zero));
  ForceLocal force_local{ctx, 1};
  ctx->call.index_bits = 15;  // (not 16: the span pass counts the bits 8-15 digit too -- the density is not known yet)
  giql_side none = *side;
  none.n = 0;
  none.chrom = none.start = none.end = nullptr;
  // the span pass of the ordinary plan, this table as its side B: per-chromosome range, length range, the digits
  // of the aligned keys (all but the lowest matter: buckets narrower than 2^16 keys sort on bits 8-15 as well)
  GIQL_TRY(run_spans(ctx, st, none, *side, n_chrom, lb, 1, hist));
  GIQL_TRY(read_meta(ctx, st));
  const DevMeta& m = *ctx->h_meta;
  if (!m.aligned_ok)
    return set_err(GIQL_ERR_STATE, "the table does not take the aligned axis (a negative coordinate, or more than 255 2^24-position blocks)");
  if (m.len_min_b <= 0) return set_err(GIQL_ERR_STATE, "the table holds irregular rows (canonical end <= start): not indexable");
  if (m.len_max_b > (int)BS_FUSE_WCAP)
    return set_err(GIQL_ERR_STATE, "a row of %d positions is longer than the bucket stage's windows allow (%u)", m.len_max_b, BS_FUSE_WCAP);
  const double per_bucket = (double)n * 65536.0 / (double)(m.total_span ? m.total_span : 1);
  idx->wbits = ctx->sw.force_bits ? ctx->sw.force_bits : density_bits(sort_tuning(ctx), per_bucket);
  if (idx->wbits == 0)
    return set_err(GIQL_ERR_STATE, "%.0f rows per 65,536 positions: too dense for the in-LDS bucket stage (at most %.0f per %d)",
                   per_bucket, ctx->sw.local_max_bucket_rows, 1 << BS_MIN_WBITS);
  ctx->call.index_bits = idx->wbits;
  idx->general = ctx->sw.no_uniform || m.len_min_b != m.len_max_b;
  idx->uni_len = idx->general ? 0 : m.len_max_b;
  idx->len_max = m.len_max_b;
  idx->span = m.total_span;
  idx->sentinel = m.sentinel;
  GIQL_TRY(idx->key.alloc(n * sizeof(u32)));
  GIQL_TRY(idx->rid.alloc(n * sizeof(u32)));
  if (idx->general) GIQL_TRY(idx->end.alloc(n * sizeof(u32)));
  GIQL_TRY(idx->small.alloc((1024 + (size_t)n_chrom + 1) * sizeof(u32)));
  GIQL_TRY(span_digit_offsets(ctx, st, lb, hist, gbase, nullptr, nullptr, "digit offsets (index)"));
  SortBufs sb = scratch;
  sb.key[0] = idx->key;
  sb.rid[0] = idx->rid;
  sb.end[0] = idx->general ? idx->end : nullptr;
  if (!idx->general) sb.end[1] = nullptr;
  // two (three) global passes from the raw columns + every bucket sorted in LDS, in place.  Three passes end in the
  // physical buffer they did not start from: the plan says which, and the index's own arrays start as the other one
  const SortRequest build = SortRequest::rows((u32)n, gbase, status).keys_from(side, lb.abase);
  if (plan_of(ctx, sb, build).result_buf == 1) sb.flip();
  GIQL_TRY(run_sort_onesweep(ctx, st, sb, build));
  if (sb.key[0] != idx->key) return set_err(GIQL_ERR_HIP, "internal: the sort did not end in the index's buffers");
  HIP_TRY(hipMemcpyAsync(idx->small, gbase, 1024 * sizeof(u32), hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(idx->small + 1024, lb.chrom_first, ((size_t)n_chrom + 1) * sizeof(u32), hipMemcpyDeviceToDevice, st));
  {
    const int rc = read_meta(ctx, st);
    if (rc == GIQL_STATUS_RESORT)
      return set_err(GIQL_ERR_STATE, "a %d-key bucket of the table holds more rows than the bucket stage sorts (%u)", 1 << idx->wbits, BS_BIG_MAX);
    if (rc != GIQL_OK) return rc;
  }
  collect_spans(ctx);
  ctx->stats.n_b = side->n;
  ctx->stats.span = (int64_t)idx->span;
  *out = idx.release();
  return GIQL_OK;
}

// INNER join of `a` against an indexed table: pairs (row of a, row of the indexed table).  Per call: a's span pass
// (lengths only), its keys on the index's axis, its sort (grouped by bucket: two passes) and the bucket stage over
// the index's rows -- the one-call join's last stage, reading the index instead of a freshly sorted side.
// GIQL_ERR_STATE: `a` holds irregular rows or rows too long for the windows (the ordinary join answers those);
// GIQL_ERR_CAPACITY with *n_pairs set when the buffers are short.
int giql_hip_inner_join_indexed_dev(giql_hip_ctx* ctx, const giql_hip_index* idx, const giql_side* a,
                                    int32_t* row_a, int32_t* row_idx, int64_t capacity, void* stream,
                                    int64_t* n_pairs) {
  if (!ctx || !idx || !n_pairs) return set_err(GIQL_ERR_INVALID, "ctx/index/n_pairs is NULL");
  GIQL_TRY(check_side(a, "a"));
  if (idx->device != ctx->device) return set_err(GIQL_ERR_INVALID, "the index lives on device %d, the context on %d", idx->device, ctx->device);
  if (capacity < 0 || (capacity > 0 && (!row_a || !row_idx))) return set_err(GIQL_ERR_INVALID, "bad output buffers");
  *n_pairs = 0;
  GIQL_TRY(begin_call(ctx, a->n, idx->n));
  hipStream_t st = (hipStream_t)stream;
  ctx->plan.fuse_done = false;
  if (a->n == 0) return GIQL_OK;
  const size_t na = (size_t)a->n, nb = (size_t)idx->n;
  if (na > OS_MAX_ROWS) return set_err(GIQL_ERR_INVALID, "side larger than 2^30 rows");
  SortBufs sa, sq;  // a's sort; buffer 1 of the index side (only a queued bucket's block ever touches it)
  u32 *hist = nullptr, *gbase = nullptr, *status = nullptr, *flags = nullptr;
  ZeroSpan zero;
  auto carve = [&](char* base) {
    Carver c{base};
    sort_sizes(c, na, sa, true);
    sq.key[1] = c.take<u32>(nb);
    sq.rid[1] = c.take<u32>(nb);
    sq.end[1] = idx->general ? c.take<u32>(nb) : nullptr;
    c.open_zeroed();
    hist = c.take<u32>((size_t)LIN_HIST_REPLICAS * 1024);
    gbase = c.take<u32>(1024);
    flags = c.take<u32>(64);
    status = c.take<u32>(4 * os_pass_words(na));
    zero = c.close_zeroed();
    return c.off;
  };
  GIQL_TRY(claim_arena(ctx, st, carve));
  ZeroedScope zeroed_scope{ctx};
  GIQL_TRY(zero_span(ctx, st, zero));
  const u32* first = idx->small + 1024;
  u32* const dead = flags;           // rows of a that cannot match (sorted last, skipped by the windows)
  u32* const irregular = flags + 1;
  int* const len_max_q = reinterpret_cast<int*>(flags + 2);
  int* const len_max_u = reinterpret_cast<int*>(flags + 3);
  {
    Phase ph(ctx, st, GIQL_PH_LINEARIZE, 3);
    hipLaunchKernelGGL(k_init_minmax, dim3(1), dim3(256), 0, st, (int*)nullptr, (int*)nullptr, 0, ctx->d_meta);
    u32 grid = cdiv((u64)na, LIN_NT);
    if (grid > (u32)LIN_MAX_BLOCKS) grid = LIN_MAX_BLOCKS;
    hipLaunchKernelGGL(k_index_query_keys, dim3(grid), dim3(LIN_NT), 0, st, a->chrom, a->start, a->end, (u32)na,
                       a->start_off, a->end_off, idx->n_chrom, first, idx->sentinel, sa.key[0], sa.end[0], dead, irregular,
                       len_max_q, hist);
    hipLaunchKernelGGL(k_digit_offsets, dim3(4), dim3(256), 0, st, hist, (u32)LIN_HIST_REPLICAS, gbase);
    GIQL_TRY(post_launch("query keys (index)"));
  }
  HIP_TRY(hipMemcpyAsync(len_max_u, &idx->len_max, sizeof(int), hipMemcpyHostToDevice, st));
  // grouped by bucket only (two passes): the windows are computed under the same mask.  The general form ranks a
  // window's keys against the bucket rows and wants them fully sorted.
  // (narrower buckets: grouped by key >> 8, three passes)
  const int q_skip = idx->general ? 0 : (idx->wbits == 16 ? 2 : 1);
  {
    ForceLocal global_only{ctx, -1};  // a's own sort: global passes only (its bucket stage would reuse the context's boundary arrays)
    GIQL_TRY(run_sort_onesweep(ctx, st, sa, SortRequest::rows((u32)na, gbase, status).skipping_digits(q_skip)));
  }
  const FuseTarget out{row_a, row_idx, (u64)capacity};
  const FuseCount fc = make_fuse_count(ctx, FuseQuery{&sa, na, dead, gbase, len_max_q}, idx->general ? 1 : 1 - idx->uni_len,
                                       skip_mask(q_skip), &out, idx->general, len_max_u, flags + 8);
  SortBufs sb = sq;
  sb.key[0] = idx->key;
  sb.rid[0] = idx->rid;
  sb.end[0] = idx->end;
  ctx->call.last_sort_local = true;
  GIQL_TRY(launch_bucket_stage(ctx, st, sb, plan_fused_stage(idx->wbits, (u32)nb, fc.kind(), fc.nq_total), (u32)nb,
                               idx->small, &fc));
  GIQL_TRY(post_launch("bucket stage (index)"));
  u32 h_flags[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(h_flags, flags, sizeof(h_flags), hipMemcpyDeviceToHost, st));
  {
    const int rc = read_meta(ctx, st);   // (synchronises the stream: h_flags has arrived too)
    if (rc == GIQL_STATUS_RESORT) return set_err(GIQL_ERR_STATE, "a bucket of the index is too large for the bucket stage");
    if (rc != GIQL_OK) return rc;
  }
  collect_spans(ctx);
  if (h_flags[1]) return set_err(GIQL_ERR_STATE, "the query table holds irregular rows (canonical end <= start): use the ordinary join");
  if ((int)h_flags[2] > (int)BS_FUSE_WCAP)
    return set_err(GIQL_ERR_STATE, "a query row of %d positions is longer than the bucket stage's windows allow (%u): use the ordinary join",
                   (int)h_flags[2], BS_FUSE_WCAP);
  const u64 total = ctx->h_meta->n_out;
  *n_pairs = (int64_t)total;
  ctx->stats.n_out = (int64_t)total;
  ctx->stats.span = (int64_t)idx->span;
  ctx->stats.reserved = idx->general ? 0 : 1;
  ctx->stats.phase_bytes[GIQL_PH_SORT_LOCAL] += (int64_t)8 * (int64_t)total;
  if (total > (u64)capacity)
    return set_err(GIQL_ERR_CAPACITY, "capacity %lld < %llu pairs", (long long)capacity, (unsigned long long)total);
  return GIQL_OK;
}

// ------------------------------------------- per-row operators against an index
// What COUNT / SEMI / ANTI read of an index beyond its sorted start keys (index_rows_kernels.hip.h): a directory of
// bucket boundaries over them and, in the general form, the end keys alone, sorted, with a directory of their own.
// Built once per index, on the first row-operator call (or by giql_hip_index_prepare_rows_dev), into buffers of the
// index's own; key / end / rid are only read.  The caller has run begin_call; the arena is claimed here and free
// again on return.
// bytes of building a directory: every cell written once, behind a search of ~log2(rows per top digit) keys
static int64_t index_directory_bytes(const giql_hip_index* idx) {
  return (int64_t)((size_t)bs_n_buckets((u32)idx->wbits) + 1) * (4 + 4 * 24);
}

// The directory over the index's start keys, which the row operators and NEAREST both read: built by whichever
// preparation runs first (stream-ordered: later kernels on `st` see it), found there by the other.
static int index_ensure_key_directory(giql_hip_ctx* ctx, giql_hip_index* idx, hipStream_t st) {
  if (idx->bnd_key) return GIQL_OK;
  const size_t n_cells = (size_t)bs_n_buckets((u32)idx->wbits) + 1;
  DevArray<u32> bnd;
  GIQL_TRY(bnd.alloc(n_cells * sizeof(u32)));
  {
    Phase ph(ctx, st, GIQL_PH_AUX);
    ctx->stats.phase_bytes[GIQL_PH_AUX] += index_directory_bytes(idx);
    hipLaunchKernelGGL(k_bucket_bounds, dim3(cdiv(n_cells, 256)), dim3(256), 0, st, idx->key, idx->n,
                       idx->small + 3 * OS_BINS, bnd, (u32)idx->wbits);
    GIQL_TRY(post_launch("start directory (index)"));
  }
  idx->bnd_key = std::move(bnd);
  return GIQL_OK;
}

static int index_prepare_rows_core(giql_hip_ctx* ctx, giql_hip_index* idx, hipStream_t st) {
  const size_t n = idx->n;
  const u32 wbits = (u32)idx->wbits;
  const size_t n_cells = (size_t)bs_n_buckets(wbits) + 1;
  DevArray<u32> end_sorted, bnd_end;  // built here (released on every early way out), moved into the index last
  GIQL_TRY(index_ensure_key_directory(ctx, idx, st));
  const int64_t dir_bytes = index_directory_bytes(idx);
  if (idx->general) {
    GIQL_TRY(end_sorted.alloc(n * sizeof(u32)));
    GIQL_TRY(bnd_end.alloc(n_cells * sizeof(u32)));
    SortBufs se;  // a keys-only sort: buffer 0 = the index's new array, buffer 1 in the arena
    u32 *hist = nullptr, *gbase = nullptr, *status = nullptr;
    auto carve = [&](char* base) {
      Carver c{base};
      se.key[1] = c.take<u32>(n);
      hist = c.take<u32>((size_t)LIN_HIST_REPLICAS * 1024);
      gbase = c.take<u32>(1024);
      status = c.take<u32>(4 * os_pass_words(n));
      return c.off;
    };
    GIQL_TRY(claim_arena(ctx, st, carve));
    se.key[0] = end_sorted;
    se.end[0] = se.end[1] = se.rid[0] = se.rid[1] = nullptr;
    // global passes only.  The plan says in which physical buffer they end: the rows start in the index's new array
    // when that is where they end, in the arena's otherwise
    const SortRequest end_sort = SortRequest::rows((u32)n, gbase, status);
    ForceLocal global_only{ctx, -1};  // (until the sort below has run; nothing else in between sorts)
    if (plan_of(ctx, se, end_sort).result_buf == 1) se.flip();
    HIP_TRY(hipMemsetAsync(hist, 0, (size_t)LIN_HIST_REPLICAS * 1024 * sizeof(u32), st));
    {
      Phase ph(ctx, st, GIQL_PH_AUX);  // the copy of the end keys the sort starts from: read once, written once
      ctx->stats.phase_bytes[GIQL_PH_AUX] += (int64_t)8 * n;
      HIP_TRY(hipMemcpyAsync(se.key[0], idx->end, n * sizeof(u32), hipMemcpyDeviceToDevice, st));
    }
    {
      Phase ph(ctx, st, GIQL_PH_SORT_HIST, 3);  // the end keys' digit histogram: every key read once
      ctx->stats.phase_bytes[GIQL_PH_SORT_HIST] += (int64_t)4 * n;
      hipLaunchKernelGGL(k_init_minmax, dim3(1), dim3(256), 0, st, (int*)nullptr, (int*)nullptr, 0, ctx->d_meta);
      u32 grid = cdiv(n, IR_NT);
      if (grid > (u32)LIN_MAX_BLOCKS) grid = LIN_MAX_BLOCKS;
      hipLaunchKernelGGL(k_hist_u32, dim3(grid), dim3(IR_NT), 0, st, idx->end, (u32)n, hist, (u32)LIN_HIST_REPLICAS);
      hipLaunchKernelGGL(k_digit_offsets, dim3(4), dim3(256), 0, st, hist, (u32)LIN_HIST_REPLICAS, gbase);
      GIQL_TRY(post_launch("end-key digits (index)"));
    }
    GIQL_TRY(run_sort_onesweep(ctx, st, se, end_sort));
    if (se.key[0] != end_sorted) return set_err(GIQL_ERR_HIP, "internal: the sort did not end in the index's buffer");
    {
      Phase ph(ctx, st, GIQL_PH_AUX);
      ctx->stats.phase_bytes[GIQL_PH_AUX] += dir_bytes;
      hipLaunchKernelGGL(k_bucket_bounds, dim3(cdiv(n_cells, 256)), dim3(256), 0, st, end_sorted, (u32)n,
                         gbase + 3 * OS_BINS, bnd_end, wbits);
      GIQL_TRY(post_launch("end directory (index)"));
    }
    GIQL_TRY(read_meta(ctx, st));  // (a look-back timeout of the sort; synchronises the stream)
  } else {
    HIP_TRY(hipStreamSynchronize(st));
  }
  idx->end_sorted = std::move(end_sorted), idx->bnd_end = std::move(bnd_end);
  idx->rows_ready = true;
  return GIQL_OK;
}

static int index_prepare_rows(giql_hip_ctx* ctx, giql_hip_index* idx, hipStream_t st) {
  if (idx->rows_ready) return GIQL_OK;
  return with_order_fallback(ctx, [&] { return index_prepare_rows_core(ctx, idx, st); });
}

static int check_index_call(giql_hip_ctx* ctx, const giql_hip_index* idx) {
  if (!ctx || !idx) return set_err(GIQL_ERR_INVALID, "ctx/index is NULL");
  if (idx->device != ctx->device)
    return set_err(GIQL_ERR_INVALID, "the index lives on device %d, the context on %d", idx->device, ctx->device);
  return GIQL_OK;
}

int giql_hip_index_prepare_rows_dev(giql_hip_ctx* ctx, giql_hip_index* idx, void* stream) {
  GIQL_TRY(check_index_call(ctx, idx));
  if (idx->rows_ready) return GIQL_OK;
  GIQL_TRY(begin_call(ctx, 0, idx->n));
  GIQL_TRY(index_prepare_rows(ctx, idx, (hipStream_t)stream));
  collect_spans(ctx);
  ctx->stats.span = (int64_t)idx->span;
  return GIQL_OK;
}

static IndexRowsView rows_view_of(const giql_hip_index* idx) {
  IndexRowsView v;
  v.first = idx->small + 1024;
  v.key = idx->key;
  v.bnd_key = idx->bnd_key;
  v.end_key = idx->general ? idx->end_sorted : nullptr;
  v.bnd_end = idx->general ? idx->bnd_end : nullptr;
  v.n = idx->n;
  v.n_chrom = idx->n_chrom;
  v.wbits = (u32)idx->wbits;
  v.uni_len = idx->uni_len;
  return v;
}

// bytes of the row kernel: the row's three columns, two directory cells per search and one key per step of a search
// inside an average bucket
static int64_t index_rows_bytes(const giql_hip_index* idx, size_t na, int out_bytes) {
  const double per_bucket = (double)idx->n / (double)bs_n_buckets((u32)idx->wbits);
  int steps = 1;
  while ((double)(1u << steps) < per_bucket + 1.0 && steps < 31) steps++;
  return (int64_t)na * (12 + out_bytes + 2 * (8 + 4 * steps));
}

// The prologue COUNT / SEMI / ANTI / NEAREST against an index share: checks, begin_call, the sizes, then `prepare`
// (index_prepare_rows / index_prepare_nearest: what the operator reads of the index) unless the query is empty.
static int index_prepare_nearest(giql_hip_ctx* ctx, giql_hip_index* idx, hipStream_t st);
static int begin_indexed_call(giql_hip_ctx* ctx, giql_hip_index* idx, const giql_side* a, hipStream_t st,
                              int (*prepare)(giql_hip_ctx*, giql_hip_index*, hipStream_t), size_t max_rows = SIZE_MAX) {
  GIQL_TRY(check_index_call(ctx, idx));
  GIQL_TRY(check_side(a, "a"));
  if ((size_t)a->n > max_rows) return set_err(GIQL_ERR_INVALID, "side larger than 2^30 rows");
  GIQL_TRY(begin_call(ctx, a->n, idx->n));
  if (a->n == 0) return GIQL_OK;
  return prepare(ctx, idx, st);
}

static int finish_index_rows_call(giql_hip_ctx* ctx, const giql_hip_index* idx, hipStream_t st) {
  GIQL_TRY(read_meta(ctx, st));
  collect_spans(ctx);
  ctx->stats.span = (int64_t)idx->span;
  ctx->stats.reserved = idx->general ? 0 : 1;
  if (ctx->h_meta->aux0)
    return set_err(GIQL_ERR_STATE, "the query table holds irregular rows (canonical end <= start): use the ordinary operator");
  return GIQL_OK;
}

int giql_hip_count_indexed_dev(giql_hip_ctx* ctx, giql_hip_index* idx, const giql_side* a, int64_t* counts_out,
                               void* stream) {
  hipStream_t st = (hipStream_t)stream;
  GIQL_TRY(begin_indexed_call(ctx, idx, a, st, index_prepare_rows));
  if (a->n == 0) return GIQL_OK;
  if (!counts_out) return set_err(GIQL_ERR_INVALID, "counts_out is NULL");
  const size_t na = (size_t)a->n;
  HIP_TRY(hipMemsetAsync(ctx->d_meta, 0, sizeof(DevMeta), st));
  {
    Phase ph(ctx, st, GIQL_PH_COUNT);
    ctx->stats.phase_bytes[GIQL_PH_COUNT] += index_rows_bytes(idx, na, 8);
    hipLaunchKernelGGL(k_index_rows<false>, dim3(cdiv(na, IR_NT)), dim3(IR_NT), 0, st, a->chrom, a->start, a->end, (u32)na,
                       a->start_off, a->end_off, rows_view_of(idx), 0, counts_out, (u32*)nullptr, &ctx->d_meta->aux0);
    GIQL_TRY(post_launch("count rows (index)"));
  }
  GIQL_TRY(finish_index_rows_call(ctx, idx, st));
  ctx->stats.n_out = a->n;
  return GIQL_OK;
}

int giql_hip_semi_anti_indexed_dev(giql_hip_ctx* ctx, giql_hip_index* idx, const giql_side* a, int anti,
                                   int32_t* rows_out, int64_t* n_out, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (ctx && idx && !n_out) return set_err(GIQL_ERR_INVALID, "n_out is NULL");
  GIQL_TRY(begin_indexed_call(ctx, idx, a, st, index_prepare_rows));
  *n_out = 0;
  if (a->n == 0) return GIQL_OK;
  if (!rows_out) return set_err(GIQL_ERR_INVALID, "rows_out is NULL");
  const size_t na = (size_t)a->n;
  u32* flag = nullptr;
  u64* bsums = nullptr;
  auto carve = [&](char* base) {
    Carver c{base};
    flag = c.take<u32>(na);
    bsums = c.take<u64>(cdiv(na, SCAN_TILE) + 2);
    return c.off;
  };
  GIQL_TRY(claim_arena(ctx, st, carve));
  HIP_TRY(hipMemsetAsync(ctx->d_meta, 0, sizeof(DevMeta), st));
  {
    Phase ph(ctx, st, GIQL_PH_COUNT);
    ctx->stats.phase_bytes[GIQL_PH_COUNT] += index_rows_bytes(idx, na, 4);
    hipLaunchKernelGGL(k_index_rows<true>, dim3(cdiv(na, IR_NT)), dim3(IR_NT), 0, st, a->chrom, a->start, a->end, (u32)na,
                       a->start_off, a->end_off, rows_view_of(idx), anti, (i64*)nullptr, flag, &ctx->d_meta->aux0);
    GIQL_TRY(post_launch("semi flags (index)"));
  }
  // as giql_hip_semi_anti_dev runs it
  GIQL_TRY(run_scan_compact(ctx, st, flag, na, bsums, bsums + cdiv(na, SCAN_TILE) + 1, rows_out, "scan + compact (index)"));
  GIQL_TRY(finish_index_rows_call(ctx, idx, st));
  *n_out = (int64_t)ctx->h_meta->n_out;
  ctx->stats.n_out = *n_out;
  ctx->stats.phase_bytes[GIQL_PH_SCAN] += (int64_t)8 * (int64_t)na + (int64_t)4 * *n_out;
  return GIQL_OK;
}

// ------------------------------------------------------ NEAREST against an index
// What NEAREST (k = 1) reads of an index beyond its sorted start keys (index_nearest_kernels.hip.h): the directory
// over them (shared with the row operators), chrom_lo[] and, in the general form, a (start, end)-ordered VIEW in
// arrays of its own -- the row ids and the prefix max of the end keys in that order, 8 bytes per row.  The index's
// key / end / rid are only read (the indexed INNER join of another context may be reading them): the short runs of
// equal start are ordered by end on COPIES (k_fix_start_ties), the end copy lives in the arena and is dropped.  A run
// longer than NEAREST_TIE_MAX (a pile-up table) declines: the index remembers it, keeps no NEAREST array and every
// NEAREST call on it returns GIQL_ERR_STATE; the other indexed operators are unaffected.  The caller has run
// begin_call; the arena is claimed here and free again on return.
static int index_nearest_declined() {
  return set_err(GIQL_ERR_STATE, "the indexed table holds a run of more than %u rows on one start: it does not take the "
                 "NEAREST form of an index; use the ordinary operator", NEAREST_TIE_MAX);
}

static int index_prepare_nearest(giql_hip_ctx* ctx, giql_hip_index* idx, hipStream_t st) {
  if (idx->nearest_state > 0) return GIQL_OK;
  if (idx->nearest_state < 0) return index_nearest_declined();
  const size_t n = idx->n;
  DevArray<u32> chrom_lo, nr_rid, nr_pmax;  // built here (released on every early way out), moved into the index last
  if (idx->general) {
    u32 *ends = nullptr, *bmax = nullptr;
    auto carve = [&](char* base) {
      Carver c{base};
      ends = c.take<u32>(n);
      bmax = c.take<u32>(cdiv(n, PM_TILE) + 1);
      return c.off;
    };
    GIQL_TRY(claim_arena(ctx, st, carve));
    GIQL_TRY(nr_rid.alloc(n * sizeof(u32)));
    GIQL_TRY(nr_pmax.alloc(n * sizeof(u32)));
    HIP_TRY(hipMemsetAsync(ctx->d_meta, 0, sizeof(DevMeta), st));
    {
      Phase ph(ctx, st, GIQL_PH_AUX);  // the copies the tie fix works on (read once, written once), the run heads' pass
      ctx->stats.phase_bytes[GIQL_PH_AUX] += (int64_t)(16 + 4) * n;
      HIP_TRY(hipMemcpyAsync(ends, idx->end, n * sizeof(u32), hipMemcpyDeviceToDevice, st));
      HIP_TRY(hipMemcpyAsync(nr_rid, idx->rid, n * sizeof(u32), hipMemcpyDeviceToDevice, st));
      hipLaunchKernelGGL(k_fix_start_ties, dim3(cdiv(n, 256)), dim3(256), 0, st, idx->key, ends, nr_rid, (u32)n,
                         ctx->d_meta);
      GIQL_TRY(post_launch("start ties (index)"));
    }
    ctx->stats.phase_bytes[GIQL_PH_AUX] += (int64_t)12 * n;  // the prefix max: read twice, written once
    GIQL_TRY(run_pmax(ctx, st, ends, (u32)n, nr_pmax, bmax));
    GIQL_TRY(read_meta(ctx, st));
    if (ctx->h_meta->aux0 != 0) {
      idx->nearest_state = -1;  // (the arrays built so far are released: the index keeps nothing of the attempt)
      return index_nearest_declined();
    }
  }
  GIQL_TRY(index_ensure_key_directory(ctx, idx, st));
  GIQL_TRY(chrom_lo.alloc(((size_t)idx->n_chrom + 1) * sizeof(u32)));
  {
    Phase ph(ctx, st, GIQL_PH_AUX);
    hipLaunchKernelGGL(k_chrom_bounds, dim3(cdiv((u64)idx->n_chrom + 1, 256)), dim3(256), 0, st, idx->small + 1024,
                       idx->n_chrom, idx->key, (u32)n, chrom_lo);
    GIQL_TRY(post_launch("chromosome ranks (index)"));
  }
  HIP_TRY(hipStreamSynchronize(st));
  idx->chrom_lo = std::move(chrom_lo), idx->nr_rid = std::move(nr_rid), idx->nr_pmax = std::move(nr_pmax);
  idx->nearest_state = 1;
  return GIQL_OK;
}

int giql_hip_index_prepare_nearest_dev(giql_hip_ctx* ctx, giql_hip_index* idx, void* stream) {
  GIQL_TRY(check_index_call(ctx, idx));
  if (idx->nearest_state > 0) return GIQL_OK;
  if (idx->nearest_state < 0) return index_nearest_declined();
  GIQL_TRY(begin_call(ctx, 0, idx->n));
  GIQL_TRY(index_prepare_nearest(ctx, idx, (hipStream_t)stream));
  collect_spans(ctx);
  ctx->stats.span = (int64_t)idx->span;
  return GIQL_OK;
}

// NEAREST k = 1 of `a` over an indexed table with the results of giql_hip_nearest_dev on the same two tables:
// neither side is sorted, nothing is scattered (k_index_nearest).
int giql_hip_nearest_indexed_dev(giql_hip_ctx* ctx, giql_hip_index* idx, const giql_side* a, int is_signed,
                                 int64_t max_distance, int32_t* idx_b_out, int64_t* dist_out, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!ctx || !idx) return set_err(GIQL_ERR_INVALID, "ctx/index is NULL");
  if (!idx_b_out || !dist_out) return set_err(GIQL_ERR_INVALID, "idx_b_out/dist_out is NULL");
  GIQL_TRY(begin_indexed_call(ctx, idx, a, st, index_prepare_nearest, OS_MAX_ROWS));
  if (a->n == 0) return GIQL_OK;
  const size_t na = (size_t)a->n;
  HIP_TRY(hipMemsetAsync(ctx->d_meta, 0, sizeof(DevMeta), st));
  IndexNearestView v;
  v.rows = rows_view_of(idx);
  v.rows.end_key = v.rows.bnd_end = nullptr;  // (the row operators' arrays: not read here, possibly not built)
  v.chrom_lo = idx->chrom_lo;
  v.rid = idx->rid;
  v.nr_pmax = idx->nr_pmax;
  v.nr_rid = idx->nr_rid;
  {
    Phase ph(ctx, st, GIQL_PH_COUNT);
    // the searches of index_rows_bytes + the candidates' keys / prefix maxima (~4 loads) and the matched row id
    ctx->stats.phase_bytes[GIQL_PH_COUNT] += index_rows_bytes(idx, na, 12) + (int64_t)na * 20;
    if (idx->general)
      hipLaunchKernelGGL(k_index_nearest<true>, dim3(cdiv(na, IR_NT)), dim3(IR_NT), 0, st, a->chrom, a->start, a->end,
                         (u32)na, a->start_off, a->end_off, v, is_signed, (i64)max_distance, idx_b_out, (i64*)dist_out,
                         &ctx->d_meta->aux1);
    else
      hipLaunchKernelGGL(k_index_nearest<false>, dim3(cdiv(na, IR_NT)), dim3(IR_NT), 0, st, a->chrom, a->start, a->end,
                         (u32)na, a->start_off, a->end_off, v, is_signed, (i64)max_distance, idx_b_out, (i64*)dist_out,
                         &ctx->d_meta->aux1);
    GIQL_TRY(post_launch("nearest (index)"));
  }
  GIQL_TRY(read_meta(ctx, st));
  collect_spans(ctx);
  ctx->stats.span = (int64_t)idx->span;
  ctx->stats.reserved = idx->general ? 0 : 1;
  if (ctx->h_meta->aux1) return set_err(GIQL_ERR_INVALID, "NEAREST: a query row has end < start");
  ctx->stats.n_out = a->n;
  return GIQL_OK;
}


// zero_upto_status: closes the carve's zeroed span where the status words begin (os_pair_sizes)
static void os_scratch_sizes(Carver& c, size_t n_max, OsScratch& o, ZeroSpan* zero_upto_status = nullptr) {
  o.hist = c.take<u32>((size_t)LIN_HIST_REPLICAS * 1024);
  o.hist_e = c.take<u32>((size_t)LIN_HIST_REPLICAS * 1024);
  o.gbase = c.take<u32>(1024);
  o.gbase_e = c.take<u32>(1024);
  if (zero_upto_status) *zero_upto_status = c.close_zeroed();
  o.status = c.take<u32>(4 * os_pass_words(n_max));
}

// The scratch of an operator that sorts both sides: A's own (its chain may run beside B's: SideChain), then B's, one
// range of the workspace that only os_pair_sizes lays out.
struct OsScratchPair {
  OsScratch a, b;
  ZeroSpan zero;  // from a's histograms to where b's status words begin (os_pair_sizes)
  // ONE memset for everything the two sides' histograms and sort passes need at zero, instead of one per histogram and
  // per sort (four launches of ~5 us on a path of ~60): the span and b's four passes of status words for n_b rows.
  // It pays for calls that sort each side ONCE: a second sort through the same status words finds them taken and
  // zeroes them again.
  int prezero(giql_hip_ctx* ctx, hipStream_t st, size_t n_b) const {
    return zero_span(ctx, st, {zero.off, zero.end + 4 * os_pass_stride(sort_tuning(ctx), n_b) * sizeof(u32)});
  }
};

// `inside`: words of the caller's that prezero() is to zero with the rest (NEAREST's digit counts of the span pass),
// carved between the two sides' scratch.
struct ExtraWords {
  u32** at;
  size_t n;
};
static void os_pair_sizes(Carver& c, size_t na, size_t nb, OsScratchPair& o, std::initializer_list<ExtraWords> inside = {}) {
  c.open_zeroed();
  os_scratch_sizes(c, na, o.a);
  for (const ExtraWords& x : inside) *x.at = c.take<u32>(x.n);
  os_scratch_sizes(c, nb, o.b, &o.zero);
}

// The tail of SEMI / ANTI: the flags compacted to ascending row ids with the count straight into DevMeta::n_out (three
// launches; were five: scan x 3, a device-to-device copy of the total, compact), then the call's last read-back.
static int finish_semi(giql_hip_ctx* ctx, hipStream_t st, const u32* flag, size_t na, u64* bsums, u64* spine_out,
                       int32_t* rows_out) {
  GIQL_TRY(run_scan_compact(ctx, st, flag, na, bsums, spine_out, rows_out, "scan + compact"));
  return read_meta(ctx, st);
}

// -------------------------------------------------------------- SEMI / ANTI
static int giql_hip_semi_anti_dev_impl(giql_hip_ctx* ctx, const giql_side* a, const giql_side* b,
                           int32_t n_chrom, int anti, int32_t* rows_out, int64_t* n_out,
                           void* stream) {
  if (!ctx || !n_out) return set_err(GIQL_ERR_INVALID, "ctx/n_out is NULL");
  GIQL_TRY(begin_pair_call(ctx, a, b, n_chrom));
  hipStream_t st = (hipStream_t)stream;
  *n_out = 0;
  if (a->n == 0) return GIQL_OK;
  if (!rows_out) return set_err(GIQL_ERR_INVALID, "rows_out is NULL");
  const size_t na = (size_t)a->n, nb = (size_t)b->n;
  GIQL_TRY(check_rows_fit(na, nb));
  const int nch = n_chrom > 0 ? n_chrom : 1;

  LinBufs lb;
  SortBufs sa, sbb;
  OsScratchPair osp;
  OsScratch &os_a = osp.a, &os = osp.b;
  u32 *flag = nullptr, *pmax = nullptr, *bmax = nullptr, *dummy_irr = nullptr;
  u64 *bsums = nullptr, *off = nullptr;
  auto carve = [&](char* base) {
    Carver c{base};
    common_sizes(c, nch, lb);
    sort_sizes(c, na, sa, true);
    sort_sizes_key_payload(c, nb ? nb : 1, sbb);  // B: (key, end)
    os_pair_sizes(c, na, nb ? nb : 1, osp);
    bsums = c.take<u64>(cdiv(na, SCAN_TILE) + 2);
    flag = c.take<u32>(na);
    off = c.take<u64>(na + 1);
    pmax = c.take<u32>(nb ? nb : 1);
    bmax = c.take<u32>(cdiv(nb ? nb : 1, PM_TILE) + 1);
    dummy_irr = c.take<u32>(16);
    return c.off;
  };
  GIQL_TRY(claim_arena(ctx, st, carve));
  ZeroedScope zeroed_scope{ctx};
  GIQL_TRY(osp.prezero(ctx, st, nb ? nb : 1));  // each side is sorted once, in either form

  GIQL_TRY(run_spans(ctx, st, *a, *b, nch, lb));
  i64 uni_len = 0;
  bool speculated = false;
  if (nb > 0) GIQL_TRY(row_form_guess(ctx, st, uni_len, speculated));
  const SortTuning tune = sort_tuning(ctx);  // (after the form guess: a first call has noted the density there)
  const bool coarse_b = nb > 0 && uni_len > 0 && coarse_b_ok(tune, nb);
  {
    // the query side's chain (linearize + sort) beside B's when it is small
    SideChain sc(ctx, st, nb > 0 ? na : 0);
    GIQL_TRY(run_linearize(ctx, sc.stream(), *a, nch, lb, Side::A, LinTarget::keys_ends(sa.key[0], sa.end[0], dummy_irr + 8),
                           LinOptions().keeping_irregular().counting_starts(os_a.starts())));
    // the query side's order only serves locality; every row keeps its real key here
    GIQL_TRY(run_sort_onesweep(ctx, sc.stream(), sa, sort_by_start(os_a, na).skipping_digits(row_skip(tune, nb))));
    if (nb > 0 && uni_len > 0) {
      // fixed-length B: keys only (its `end` column is not read again), no prefix max
      sbb.end[0] = sbb.end[1] = nullptr;
      GIQL_TRY(run_linearize(ctx, st, *b, nch, lb, Side::B, LinTarget::keys_only(sbb.key[0], dummy_irr),
                             LinOptions().keeping_irregular().counting_starts(os.starts()).without_end_column()));
      GIQL_TRY(run_sort_onesweep(ctx, st, sbb, sort_by_start(os, nb).skipping_digits(coarse_b ? 1 : 0)));
    } else if (nb > 0) {
      // every B row keeps its real key: the prefix-max test is exact for any row
      GIQL_TRY(run_linearize(ctx, st, *b, nch, lb, Side::B, LinTarget::keys_ends(sbb.key[0], sbb.end[0], dummy_irr),
                             LinOptions().keeping_irregular().counting_starts(os.starts())));
#if defined(GIQL_LIN_ABLATE)  // timing-only builds stop here: their keys / histograms are not valid
      GIQL_TRY(read_meta(ctx, st));
      collect_spans(ctx);
      return GIQL_OK;
#endif
      GIQL_TRY(run_sort_onesweep(ctx, st, sbb, sort_by_start(os, nb)));
      GIQL_TRY(run_pmax(ctx, st, sbb.end[0], (u32)nb, pmax, bmax));
    }
    GIQL_TRY(sc.join());
  }
  {
    Phase ph(ctx, st, GIQL_PH_COUNT);
    if (coarse_b)
      hipLaunchKernelGGL(k_semi_flags_uniform_coarse, dim3(cdiv(na, 256)), dim3(256), 0, st, sa.key[0], sa.end[0],
                         sa.rid[0], (u32)na, ctx->d_meta, sbb.key[0], (u32)nb, uni_len, anti, flag);
    else if (nb > 0 && uni_len > 0)
      hipLaunchKernelGGL(k_semi_flags_uniform, dim3(cdiv(na, 256)), dim3(256), 0, st, sa.key[0], sa.end[0],
                         sa.rid[0], (u32)na, ctx->d_meta, sbb.key[0], (u32)nb, uni_len, anti, flag);
    else
      hipLaunchKernelGGL(k_semi_flags, dim3(cdiv(na, 256)), dim3(256), 0, st, sa.key[0], sa.end[0],
                         sa.rid[0], (u32)na, ctx->d_meta, sbb.key[0], pmax, (u32)nb, anti, flag);
    GIQL_TRY(post_launch("semi flags"));
  }
  GIQL_TRY(finish_semi(ctx, st, flag, na, bsums, off + na, rows_out));
  if (nb > 0 && !row_form_settled(ctx, uni_len, speculated))  // B is not fixed-length after all
    return GIQL_STATUS_GUESS_MISSED;
  collect_spans(ctx);
  ctx->stats.reserved = (uni_len > 0 ? 1 : 0) | (coarse_b ? 0x10 : 0);  // form: fixed-length B or general; bit 4: B sorted coarsely (without its lowest digit)
  *n_out = (int64_t)ctx->h_meta->n_out;
  ctx->stats.n_out = *n_out;
  note_span(ctx);
  return GIQL_OK;
}

int giql_hip_semi_anti_dev(giql_hip_ctx* ctx, const giql_side* a, const giql_side* b, int32_t n_chrom,
                           int anti, int32_t* rows_out, int64_t* n_out, void* stream) {
  return with_order_fallback(ctx, [&] { return giql_hip_semi_anti_dev_impl(ctx, a, b, n_chrom, anti, rows_out, n_out, stream); });
}

// ------------------------------------------------------------------- COUNT
static int giql_hip_count_dev_impl(giql_hip_ctx* ctx, const giql_side* a, const giql_side* b, int32_t n_chrom,
                       int64_t* counts_out, void* stream) {
  if (!ctx) return set_err(GIQL_ERR_INVALID, "ctx is NULL");
  GIQL_TRY(begin_pair_call(ctx, a, b, n_chrom));
  hipStream_t st = (hipStream_t)stream;
  if (a->n == 0) return GIQL_OK;
  if (!counts_out) return set_err(GIQL_ERR_INVALID, "counts_out is NULL");
  const size_t na = (size_t)a->n, nb = (size_t)b->n;
  GIQL_TRY(check_rows_fit(na, nb));
  if (nb == 0 || n_chrom == 0) {
    HIP_TRY(hipMemsetAsync(counts_out, 0, na * sizeof(int64_t), st));
    return GIQL_OK;
  }
  LinBufs lb;
  SortBufs sa, sstart, send;
  OsScratchPair osp;
  OsScratch &os_a = osp.a, &os = osp.b;
  u32 *irr_a_list = nullptr, *irr_b_list = nullptr;
  auto carve = [&](char* base) {
    Carver c{base};
    common_sizes(c, n_chrom, lb);
    sort_sizes(c, na, sa, true);
    sort_sizes_starts_ends(c, nb, sstart, send);
    os_pair_sizes(c, na, nb, osp);
    irr_a_list = c.take<u32>(na);
    irr_b_list = c.take<u32>(nb);
    return c.off;
  };
  GIQL_TRY(claim_arena(ctx, st, carve));

  GIQL_TRY(run_spans(ctx, st, *a, *b, n_chrom, lb));
  i64 uni_len = 0;
  bool speculated = false;
  GIQL_TRY(row_form_guess(ctx, st, uni_len, speculated));
  const SortTuning tune = sort_tuning(ctx);  // (after the form guess: a first call has noted the density there)
  const bool coarse_b = uni_len > 0 && coarse_b_ok(tune, nb);
  ZeroedScope zeroed_scope{ctx};
  // (a choice of speed: the general form sorts B twice through one set of status words, and its second sort would
  // find them taken and zero them itself all the same)
  if (uni_len > 0) GIQL_TRY(osp.prezero(ctx, st, nb));
  {
    SideChain sc(ctx, st, na);
    GIQL_TRY(run_linearize(ctx, sc.stream(), *a, n_chrom, lb, Side::A, LinTarget::keys_ends(sa.key[0], sa.end[0], irr_a_list),
                           LinOptions().counting_starts(os_a.starts())));
    // locality only: k_count_rows tells irregular rows by their key
    GIQL_TRY(run_sort_onesweep(ctx, sc.stream(), sa, sort_by_start(os_a, na).skipping_digits(row_skip(tune, nb))));
    if (uni_len > 0) {
      // fixed-length B: one sorted array (its sorted ends are its sorted starts + L)
      GIQL_TRY(run_linearize(ctx, st, *b, n_chrom, lb, Side::B, LinTarget::keys_only(sstart.key[0], irr_b_list),
                             LinOptions().counting_starts(os.starts()).without_end_column()));
      GIQL_TRY(run_sort_onesweep(ctx, st, sstart, sort_by_start(os, nb).skipping_digits(coarse_b ? 1 : 0)));
    } else {
      GIQL_TRY(run_linearize(ctx, st, *b, n_chrom, lb, Side::B, LinTarget::keys_ends(sstart.key[0], send.key[0], irr_b_list),
                             LinOptions().counting_starts(os.starts()).counting_ends(os.ends())));
      GIQL_TRY(run_sort_onesweep(ctx, st, sstart, sort_by_start(os, nb)));
      GIQL_TRY(run_sort_onesweep(ctx, st, send, sort_by_end(os, nb)));
    }
    GIQL_TRY(sc.join());
  }
  {
    Phase ph(ctx, st, GIQL_PH_COUNT);
    hipLaunchKernelGGL(k_count_rows, dim3(cdiv(na, 256)), dim3(256), 0, st, sa.key[0], sa.end[0],
                       sa.rid[0], (u32)na, view_of(*a), view_of(*b), sstart.key[0], send.key[0], (u32)nb,
                       irr_b_list, ctx->d_meta, counts_out, uni_len, coarse_b ? 1 : 0);
    GIQL_TRY(post_launch("count rows"));
  }
  GIQL_TRY(read_meta(ctx, st));
  if (!row_form_settled(ctx, uni_len, speculated))  // B is not fixed-length after all
    return GIQL_STATUS_GUESS_MISSED;
  ctx->stats.reserved = (uni_len > 0 ? 1 : 0) | (coarse_b ? 0x10 : 0);
  ctx->stats.n_irregular_a = ctx->h_meta->irr_a;
  ctx->stats.n_irregular_b = ctx->h_meta->irr_b;
  if (ctx->h_meta->irr_a > 0) {
    Phase ph(ctx, st, GIQL_PH_IRREGULAR);
    hipLaunchKernelGGL(k_count_irregular, dim3(ctx->h_meta->irr_a), dim3(256), 0, st, view_of(*a),
                       view_of(*b), irr_a_list, counts_out);
    GIQL_TRY(post_launch("count irregular"));
    HIP_TRY(hipStreamSynchronize(st));
  }
  collect_spans(ctx);
  ctx->stats.n_out = a->n;
  note_span(ctx);
  return GIQL_OK;
}

int giql_hip_count_dev(giql_hip_ctx* ctx, const giql_side* a, const giql_side* b, int32_t n_chrom,
                       int64_t* counts_out, void* stream) {
  return with_order_fallback(ctx, [&] { return giql_hip_count_dev_impl(ctx, a, b, n_chrom, counts_out, stream); });
}

// ----------------------------------------------------------------- NEAREST
// out32 (giql_hip_nearest32_dev): [n_a] {idx_b, distance} int32 records instead of the two arrays
static int giql_hip_nearest_dev_impl(giql_hip_ctx* ctx, const giql_side* a, const giql_side* b, int32_t n_chrom,
                         int is_signed, int64_t max_distance, int32_t* idx_b_out, int64_t* dist_out,
                         void* stream, int32_t* out32 = nullptr) {
  if (!ctx) return set_err(GIQL_ERR_INVALID, "ctx is NULL");
  GIQL_TRY(begin_pair_call(ctx, a, b, n_chrom));
  hipStream_t st = (hipStream_t)stream;
  if (a->n == 0) return GIQL_OK;
  if (!out32 && (!idx_b_out || !dist_out)) return set_err(GIQL_ERR_INVALID, "idx_b_out/dist_out is NULL");
  if (out32 && ((uintptr_t)out32 & 7)) return set_err(GIQL_ERR_INVALID, "idx_dist_out must be 8-byte aligned");
  const size_t na = (size_t)a->n, nb = (size_t)b->n;
  GIQL_TRY(check_rows_fit(na, nb));
  if (nb == 0 || n_chrom == 0) {
    if (out32) {
      hipLaunchKernelGGL(k_nearest32_none, dim3(cdiv(na, 256)), dim3(256), 0, st, reinterpret_cast<int2*>(out32), (u32)na);
      return post_launch("nearest32 (no target)");
    }
    HIP_TRY(hipMemsetAsync(idx_b_out, 0xFF, na * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(dist_out, 0, na * sizeof(int64_t), st));
    return GIQL_OK;
  }
  LinBufs lb;
  SortBufs sa, sbb;
  OsScratchPair osp;
  OsScratch &os_a = osp.a, &os = osp.b;
  u32 *pmax = nullptr, *bmax = nullptr, *dummy_irr = nullptr, *chrom_lo = nullptr;
  NearestRec* recs = nullptr;
  auto carve = [&](char* base) {
    Carver c{base};
    common_sizes(c, n_chrom, lb);
    sort_sizes(c, na, sa, true);
    sort_sizes(c, nb, sbb, true);
    const size_t top_words = (size_t)LIN_HIST_REPLICAS * MM_TOP_WORDS;  // the span pass's digit counts: zeroed with the rest
    os_pair_sizes(c, na, nb, osp,
                  {{&lb.top_partial, top_words}, {&lb.top_partial2, top_words}, {&lb.abase, (size_t)MM_HIST_CHROMS}});
    recs = c.take<NearestRec>(out32 ? 0 : na);   // (the 32-bit form scatters its records straight into the output)
    pmax = c.take<u32>(nb);
    bmax = c.take<u32>(cdiv(nb, PM_TILE) + 1);
    chrom_lo = c.take<u32>((size_t)n_chrom + 2);
    dummy_irr = c.take<u32>(16);
    return c.off;
  };
  GIQL_TRY(claim_arena(ctx, st, carve));

  const bool two_sorts = ctx->guess.nearest_two_sorts;
  ZeroedScope zeroed_scope{ctx};
  // (a choice of speed: the two-sort plan reuses B's status words, its second sort would zero them itself all the same)
  if (!two_sorts) GIQL_TRY(osp.prezero(ctx, st, nb));
  // Both sides sorted from their raw columns (round 3): with every chromosome base a multiple of 2^24 the span pass
  // counts the digits of the keys itself (k_chrom_minmax<1>, "Histogram in the span pass"), and the first sort pass
  // of each side builds key and end key from (chrom, start, end) -- no linearize pass (2 x 49 us at 10M x 10M against
  // ~2 x 22 more in the span pass and the first sort pass).  Every NEAREST row keeps its real key, zero-length rows
  // included, so the only guess is the layout: taken when the previous call's data took it, validated at the
  // read-back; a first call probes it (digits counted for B only) and sorts the ordinary way.
  const SortTuning tune = sort_tuning(ctx);
  const bool hist_ok = !two_sorts && ctx->call.zeroed.covers(os.hist, HIST_BYTES) && !ctx->sw.no_span_hist && ctx->sw.os_variant == 0 &&
                       n_chrom <= MM_HIST_CHROMS && !sort_is_local(tune, na) && !sort_is_local(tune, nb);
  const bool keygen = hist_ok && ctx->guess.nearest_aligned == 1;
  const bool probe = hist_ok && ctx->guess.nearest_aligned == -1;
  if (keygen) lb.hist_partial2 = os_a.hist;
  if (!(keygen || probe)) lb.abase = nullptr;  // (run_spans: no digit counting)
  GIQL_TRY(run_spans(ctx, st, *a, *b, n_chrom, lb, (keygen || probe) ? 1 : -1, os.hist));
  if (keygen) {
    Phase ph(ctx, st, GIQL_PH_LINEARIZE, 2);
    hipLaunchKernelGGL(k_fold_top2, dim3(MM_HIST_CHROMS, 2), dim3(256), 0, st, lb.top_partial, lb.top_partial2, lb.abase,
                       os.hist, os_a.hist);
    hipLaunchKernelGGL(k_digit_offsets2, dim3(4, 2), dim3(256), 0, st, os.hist, os_a.hist, (u32)LIN_HIST_REPLICAS,
                       os.gbase, os_a.gbase);
    GIQL_TRY(post_launch("digit offsets (span histogram, NEAREST)"));
  }
  SideChain sc(ctx, st, na);
  if (!keygen)
    GIQL_TRY(run_linearize(ctx, sc.stream(), *a, n_chrom, lb, Side::A, LinTarget::keys_ends(sa.key[0], sa.end[0], dummy_irr + 8),
                           LinOptions().keeping_irregular().counting_starts(os_a.starts())));
  // the query side's order only serves locality; every row keeps its real key here
  GIQL_TRY(run_sort_onesweep(ctx, sc.stream(), sa,
                             sort_by_start(os_a, na).keys_from(keygen ? a : nullptr, lb.abase)
                                 .skipping_digits(row_skip(tune, nb))));
  if (!keygen)
    GIQL_TRY(run_linearize(ctx, st, *b, n_chrom, lb, Side::B, LinTarget::keys_ends(sbb.key[0], sbb.end[0], dummy_irr),
                           LinOptions().keeping_irregular().counting_starts(os.starts())
                               .counting_ends(two_sorts ? os.ends() : DigitCounts())));
  // (an inverted B row -- NEAREST needs start <= end on both sides -- is reported by the span pass: DevMeta::inverted_b)
  if (two_sorts) {
    GIQL_TRY(run_sort_two_keys(ctx, st, sbb, (u32)nb, os));  // (start, end) order
  } else {
    // one sort by start; the (short) runs of equal starts are ordered by end in place
    GIQL_TRY(run_sort_onesweep(ctx, st, sbb, sort_by_start(os, nb).keys_from(keygen ? b : nullptr, lb.abase)));
    Phase ph(ctx, st, GIQL_PH_AUX);
    hipLaunchKernelGGL(k_fix_start_ties, dim3(cdiv(nb, 256)), dim3(256), 0, st, sbb.key[0], sbb.end[0],
                       sbb.rid[0], (u32)nb, ctx->d_meta);
  }
  GIQL_TRY(run_pmax(ctx, st, sbb.end[0], (u32)nb, pmax, bmax));
  GIQL_TRY(sc.join());
  {
    Phase ph(ctx, st, GIQL_PH_COUNT, 3);
    hipLaunchKernelGGL(k_chrom_bounds, dim3(cdiv((u64)n_chrom + 1, 256)), dim3(256), 0, st,
                       lb.chrom_first, n_chrom, sbb.key[0], (u32)nb, chrom_lo);
    if (out32) {
      hipLaunchKernelGGL(k_nearest<true>, dim3(cdiv(na, NR_TQ)), dim3(NR_NT), 0, st, sa.key[0], sa.end[0], sa.rid[0],
                         (u32)na, n_chrom, lb.chrom_first, chrom_lo, sbb.key[0], pmax, sbb.rid[0], (u32)nb,
                         is_signed, (i64)max_distance, (NearestRec*)nullptr, ctx->d_meta, reinterpret_cast<int2*>(out32));
    } else {
      hipLaunchKernelGGL(k_nearest<false>, dim3(cdiv(na, NR_TQ)), dim3(NR_NT), 0, st, sa.key[0], sa.end[0], sa.rid[0],
                         (u32)na, n_chrom, lb.chrom_first, chrom_lo, sbb.key[0], pmax, sbb.rid[0], (u32)nb,
                         is_signed, (i64)max_distance, recs, ctx->d_meta, (int2*)nullptr);
      hipLaunchKernelGGL(k_nearest_unpack, dim3(cdiv(na, 256)), dim3(256), 0, st, recs, (u32)na, idx_b_out,
                         (i64*)dist_out);
    }
    GIQL_TRY(post_launch("nearest"));
  }
  GIQL_TRY(read_meta(ctx, st));
  if (keygen || probe) {
    const bool aligned_now = ctx->h_meta->aligned_ok != 0;
    ctx->guess.nearest_aligned = aligned_now ? 1 : 0;
    if (keygen && !aligned_now)  // the layout did not hold for this data: its keys were built on bases that overlap
      return GIQL_STATUS_GUESS_MISSED;
  }
  if (ctx->h_meta->inverted_b) return set_err(GIQL_ERR_INVALID, "NEAREST: a target row has end < start");
  if (!two_sorts && ctx->h_meta->aux0 != 0) {
    // a long run of equal starts (pile-ups): this table wants the two-sort plan
    ctx->guess.nearest_two_sorts = true;
    return GIQL_STATUS_GUESS_MISSED;
  }
  if (out32 && ctx->h_meta->aux1 != 0)
    return set_err(GIQL_ERR_INVALID, "NEAREST: a distance does not fit int32; use giql_hip_nearest_dev (int64 distances)");
  collect_spans(ctx);
  ctx->stats.n_out = a->n;
  note_span(ctx);
  return GIQL_OK;
}

int giql_hip_nearest_dev(giql_hip_ctx* ctx, const giql_side* a, const giql_side* b, int32_t n_chrom,
                         int is_signed, int64_t max_distance, int32_t* idx_b_out, int64_t* dist_out,
                         void* stream) {
  return with_order_fallback(ctx, [&] { return giql_hip_nearest_dev_impl(ctx, a, b, n_chrom, is_signed, max_distance, idx_b_out, dist_out, stream); });
}


int giql_hip_nearest32_dev(giql_hip_ctx* ctx, const giql_side* a, const giql_side* b, int32_t n_chrom, int is_signed,
                           int64_t max_distance, int32_t* idx_dist_out, void* stream) {
  if (!idx_dist_out && a && a->n > 0) return set_err(GIQL_ERR_INVALID, "idx_dist_out is NULL");
  return with_order_fallback(ctx, [&] { return giql_hip_nearest_dev_impl(ctx, a, b, n_chrom, is_signed, max_distance, nullptr, nullptr, stream, idx_dist_out); });
}

// ------------------------------------------------------------ NEAREST k > 1
static int giql_hip_nearest_k_dev_impl(giql_hip_ctx* ctx, const giql_side* a, const giql_side* b, int32_t n_chrom,
                                       int32_t k, int is_signed, int64_t max_distance, int32_t* idx_b_out,
                                       int64_t* dist_out, void* stream) {
  if (!ctx) return set_err(GIQL_ERR_INVALID, "ctx is NULL");
  if (k < 1 || k > NEAREST_K_MAX) return set_err(GIQL_ERR_INVALID, "k=%d outside [1, %d]", k, NEAREST_K_MAX);
  GIQL_TRY(begin_pair_call(ctx, a, b, n_chrom));
  hipStream_t st = (hipStream_t)stream;
  if (a->n == 0) return GIQL_OK;
  if (!idx_b_out || !dist_out) return set_err(GIQL_ERR_INVALID, "idx_b_out/dist_out is NULL");
  const size_t na = (size_t)a->n, nb = (size_t)b->n;
  GIQL_TRY(check_rows_fit(na, nb));
  if (na * (size_t)k > 0x7FFFFFF0ull) return set_err(GIQL_ERR_INVALID, "n_a * k does not fit 31 bits");
  if (nb == 0 || n_chrom == 0) {
    HIP_TRY(hipMemsetAsync(idx_b_out, 0xFF, na * k * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(dist_out, 0, na * k * sizeof(int64_t), st));
    return GIQL_OK;
  }
  LinBufs lb;
  SortBufs sa, sbb, se;
  OsScratch os;
  u32 *pmax = nullptr, *bmax = nullptr, *dummy_irr = nullptr, *chrom_lo = nullptr, *chrom_lo_e = nullptr;
  NearestRec* recs = nullptr;
  auto carve = [&](char* base) {
    Carver c{base};
    common_sizes(c, n_chrom, lb);
    sort_sizes(c, na, sa, true);
    sort_sizes(c, nb, sbb, true);
    sort_sizes(c, nb, se, true);   // the (end, start) order: key = end, "end" payload = start
    os_scratch_sizes(c, na > nb ? na : nb, os);
    recs = c.take<NearestRec>(na * (size_t)k);
    pmax = c.take<u32>(nb);
    bmax = c.take<u32>(cdiv(nb, PM_TILE) + 1);
    chrom_lo = c.take<u32>((size_t)n_chrom + 2);
    chrom_lo_e = c.take<u32>((size_t)n_chrom + 2);
    dummy_irr = c.take<u32>(16);
    return c.off;
  };
  GIQL_TRY(claim_arena(ctx, st, carve));

  GIQL_TRY(run_spans(ctx, st, *a, *b, n_chrom, lb));
  // Two sorted views of B from ONE linearize pass (it counts the digits of the starts and of the ends):
  //   by (start, end) and by (end, start).
  GIQL_TRY(run_linearize(ctx, st, *b, n_chrom, lb, Side::B, LinTarget::keys_ends(sbb.key[0], sbb.end[0], dummy_irr),
                         LinOptions().keeping_irregular().counting_starts(os.starts()).counting_ends(os.ends())));
  const bool two_sorts = ctx->guess.nearest_two_sorts;
  if (two_sorts) {
    // tables with long runs of equal starts or ends: stable two-key sorts -- (start, end) = by end, then stably by
    // start; (end, start) = that order stably re-sorted by end
    GIQL_TRY(run_sort_two_keys(ctx, st, sbb, (u32)nb, os));
    HIP_TRY(hipMemcpyAsync(se.key[0], sbb.end[0], nb * sizeof(u32), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(se.end[0], sbb.key[0], nb * sizeof(u32), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(se.rid[0], sbb.rid[0], nb * sizeof(u32), hipMemcpyDeviceToDevice, st));
    GIQL_TRY(run_sort_onesweep(ctx, st, se, sort_by_end(os, nb).keeping_rids()));
  } else {
    // ONE sort per view (eight passes instead of twelve): each view sorted on its first key from the linearized
    // columns, the -- short -- runs of equal first keys ordered by the second key in place (k_fix_start_ties; a run
    // too long for that flags the table for the two-key plan above, as in NEAREST k = 1)
    HIP_TRY(hipMemcpyAsync(se.key[0], sbb.end[0], nb * sizeof(u32), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(se.end[0], sbb.key[0], nb * sizeof(u32), hipMemcpyDeviceToDevice, st));
    GIQL_TRY(run_sort_onesweep(ctx, st, sbb, sort_by_start(os, nb)));
    GIQL_TRY(run_sort_onesweep(ctx, st, se, sort_by_end(os, nb)));
    Phase ph(ctx, st, GIQL_PH_AUX, 2);
    hipLaunchKernelGGL(k_fix_start_ties, dim3(cdiv(nb, 256)), dim3(256), 0, st, sbb.key[0], sbb.end[0], sbb.rid[0],
                       (u32)nb, ctx->d_meta);
    hipLaunchKernelGGL(k_fix_start_ties, dim3(cdiv(nb, 256)), dim3(256), 0, st, se.key[0], se.end[0], se.rid[0],
                       (u32)nb, ctx->d_meta);
  }
  GIQL_TRY(run_pmax(ctx, st, sbb.end[0], (u32)nb, pmax, bmax));
  GIQL_TRY(run_linearize(ctx, st, *a, n_chrom, lb, Side::A, LinTarget::keys_ends(sa.key[0], sa.end[0], dummy_irr),
                         LinOptions().keeping_irregular().counting_starts(os.starts())));
  // the query side's order only serves locality; every row keeps its real key here
  GIQL_TRY(run_sort_onesweep(ctx, st, sa, sort_by_start(os, na).skipping_digits(row_skip(sort_tuning(ctx), nb))));
  {
    Phase ph(ctx, st, GIQL_PH_COUNT, 4);
    hipLaunchKernelGGL(k_chrom_bounds, dim3(cdiv((u64)n_chrom + 1, 256)), dim3(256), 0, st, lb.chrom_first, n_chrom,
                       sbb.key[0], (u32)nb, chrom_lo);
    hipLaunchKernelGGL(k_chrom_bounds, dim3(cdiv((u64)n_chrom + 1, 256)), dim3(256), 0, st, lb.chrom_first, n_chrom,
                       se.key[0], (u32)nb, chrom_lo_e);
    if (k >= 16) {  // a row's k ids / distances are contiguous runs of 64+ / 128+ bytes: straight into the outputs
                     // (at k = 8 the two scattered 32 / 64-byte runs cost what the 128-byte records + the unpack pass do)
      hipLaunchKernelGGL(k_nearest_k<true>, dim3(cdiv(na, NR_TQ)), dim3(NR_NT), 0, st, sa.key[0], sa.end[0], sa.rid[0],
                         (u32)na, n_chrom, lb.chrom_first, chrom_lo, chrom_lo_e, sbb.key[0], sbb.end[0], pmax,
                         sbb.rid[0], se.key[0], se.end[0], se.rid[0], (u32)nb, (int)k, is_signed, (i64)max_distance,
                         recs, idx_b_out, (i64*)dist_out, ctx->d_meta);
    } else {
      hipLaunchKernelGGL(k_nearest_k<false>, dim3(cdiv(na, NR_TQ)), dim3(NR_NT), 0, st, sa.key[0], sa.end[0], sa.rid[0],
                         (u32)na, n_chrom, lb.chrom_first, chrom_lo, chrom_lo_e, sbb.key[0], sbb.end[0], pmax,
                         sbb.rid[0], se.key[0], se.end[0], se.rid[0], (u32)nb, (int)k, is_signed, (i64)max_distance,
                         recs, idx_b_out, (i64*)dist_out, ctx->d_meta);
      hipLaunchKernelGGL(k_nearest_unpack, dim3(cdiv(na * (size_t)k, 256)), dim3(256), 0, st, recs,
                         (u32)(na * (size_t)k), idx_b_out, (i64*)dist_out);
    }
    GIQL_TRY(post_launch("nearest k"));
  }
  GIQL_TRY(read_meta(ctx, st));
  if (!two_sorts && ctx->h_meta->aux0 != 0) {
    // a long run of equal starts or ends (pile-ups): this table wants the two-key sorts
    ctx->guess.nearest_two_sorts = true;
    return GIQL_STATUS_GUESS_MISSED;
  }
  if (ctx->h_meta->inverted_b) return set_err(GIQL_ERR_INVALID, "NEAREST: a target row has end < start");
  collect_spans(ctx);
  ctx->stats.n_out = a->n * (int64_t)k;
  note_span(ctx);
  return GIQL_OK;
}

int giql_hip_nearest_k_dev(giql_hip_ctx* ctx, const giql_side* a, const giql_side* b, int32_t n_chrom, int32_t k,
                           int is_signed, int64_t max_distance, int32_t* idx_b_out, int64_t* dist_out,
                           void* stream) {
  return with_order_fallback(ctx, [&] { return giql_hip_nearest_k_dev_impl(ctx, a, b, n_chrom, k, is_signed, max_distance, idx_b_out, dist_out, stream); });
}

// ------------------------------------- stages of the one-table and aggregate operators
// The status-word frame of a call whose kernels report through DevMeta::status alone: zero the word before the
// launches; after them read it back, wait, and collect the spans.  The caller words what a set word means.
static int begin_status(giql_hip_ctx* ctx, hipStream_t st) {
  HIP_TRY(hipMemsetAsync(&ctx->d_meta->status, 0, sizeof(int), st));
  return GIQL_OK;
}
static int finish_status(giql_hip_ctx* ctx, hipStream_t st, int& status) {
  status = 0;
  HIP_TRY(hipMemcpyAsync(&status, &ctx->d_meta->status, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  collect_spans(ctx);
  return GIQL_OK;
}

// The event sweep of DISJOIN's plan and of the coverage segments (disjoin_kernels.hip.h): the 2n start / end events of
// one table as keys on the linear axis -> ONE (key, id) sort -> per sorted event "the last of its key" and "a start",
// and the exclusive scans of both.  What an operator makes of the breakpoints stays in the operator.
struct EventBufs {
  LinBufs lb;
  SortBufs sb;
  OsScratch os;
  u32 *last = nullptr, *is_start = nullptr, *last_excl = nullptr, *start_excl = nullptr;
  u64 *bsums = nullptr, *n_bp = nullptr, *scratch_total = nullptr;  // carved by the operator, behind the prefix
};

// the prefix the two operators' workspaces share
static void event_sizes(Carver& c, int n_chrom, size_t nev, EventBufs& E) {
  common_sizes(c, n_chrom, E.lb);
  sort_sizes_key_rid(c, nev, E.sb);
  os_scratch_sizes(c, nev, E.os);
  E.last = c.take<u32>(nev);
  E.is_start = c.take<u32>(nev);
  E.last_excl = c.take<u32>(nev + 1);
  E.start_excl = c.take<u32>(nev + 1);
}

// t: the table whose rows the operator goes on to cut; r: the table of the events, nullptr = t itself (DISJOIN's self
// mode, coverage).  A table of no rows has no event: no key, no flag, and the sort and the scans run over nothing.
static int run_events(giql_hip_ctx* ctx, hipStream_t st, const giql_side& t, const giql_side* r, int n_chrom,
                      EventBufs& E, const char* op) {
  const giql_side& ref = r ? *r : t;
  const size_t nr = (size_t)ref.n, nev = 2 * nr;
  char what[32];
  giql_side none;
  memset(&none, 0, sizeof(none));
  GIQL_TRY(run_spans(ctx, st, t, r ? *r : none, n_chrom, E.lb));
  if (nev > 0) {
    HIP_TRY(hipMemsetAsync(E.os.hist, 0, (size_t)LIN_HIST_REPLICAS * 1024 * sizeof(u32), st));
    Phase ph(ctx, st, GIQL_PH_LINEARIZE, 2);
    ctx->stats.phase_bytes[GIQL_PH_LINEARIZE] += (int64_t)20 * nr;  // three columns read, two keys written
    u32 grid = cdiv((u64)nr, LIN_NT);
    if (grid > (u32)LIN_MAX_BLOCKS) grid = LIN_MAX_BLOCKS;
    hipLaunchKernelGGL(k_dj_events, dim3(grid), dim3(LIN_NT), 0, st, view_of(ref), n_chrom, E.lb.chrom_base,
                       E.sb.key[0], E.os.hist, ctx->d_meta, r ? DJ_BAD_REFERENCE : DJ_BAD_TARGET);
    hipLaunchKernelGGL(k_digit_offsets, dim3(4), dim3(256), 0, st, E.os.hist, (u32)LIN_HIST_REPLICAS, E.os.gbase);
    snprintf(what, sizeof(what), "%s events", op);
    GIQL_TRY(post_launch(what));
  }
  GIQL_TRY(run_sort_onesweep(ctx, st, E.sb, sort_by_start(E.os, nev)));
  if (nev > 0) {
    Phase ph(ctx, st, GIQL_PH_COUNT, 1);
    ctx->stats.phase_bytes[GIQL_PH_COUNT] += (int64_t)16 * nev;  // keys + ids read, two flags written
    hipLaunchKernelGGL(k_dj_flags, dim3(cdiv(nev, 256)), dim3(256), 0, st, E.sb.key[0], E.sb.rid[0], (u32)nev, (u32)nr,
                       E.last, E.is_start);
    snprintf(what, sizeof(what), "%s flags", op);
    GIQL_TRY(post_launch(what));
  }
  GIQL_TRY(run_scan<u32>(ctx, st, GIQL_PH_SCAN, E.last, (u64)nev, E.last_excl, E.bsums, E.n_bp));
  return run_scan<u32>(ctx, st, GIQL_PH_SCAN, E.is_start, (u64)nev, E.start_excl, E.bsums, E.scratch_total);
}

// The call's read-back: DevMeta, the `start > end` bits of k_dj_events / k_dj_count the caller looks at, the status.
static int finish_events(giql_hip_ctx* ctx, hipStream_t st, u32 bad_bits) {
  HIP_TRY(hipMemcpyAsync(ctx->h_meta, ctx->d_meta, sizeof(DevMeta), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (ctx->h_meta->aux0 & bad_bits & DJ_BAD_TARGET)
    return set_err(GIQL_ERR_INVALID, "DISJOIN needs start <= end on every row: the target has a row with start > end");
  if (ctx->h_meta->aux0 & bad_bits & DJ_BAD_REFERENCE)
    return set_err(GIQL_ERR_INVALID, "DISJOIN needs start <= end on every row: the reference has a row with start > end");
  return read_meta(ctx, st);
}

// The caller's aggregates -> the by-value kernel argument of the segmented reduction (merge_agg_kernels.hip.h).
// Aggregates over one source share one column, i.e. one gather; the kernels walk the aggregates column by column.
// over_pairs: a pair aggregate's sources (include/giql_hip_pair_expr_agg.h) -- a program over `nodes`, or a column,
// where a COUNT reads validity alone (data may be NULL; every COUNT over one validity shares a column); MERGE's are
// columns with data, keyed by (data, valid, type) whatever the function.  ordered: a float SUM, MIN or MAX -- their
// bits depend on the order of their inputs (a sum's rounding; which of +0.0 and -0.0 a MIN / MAX keeps).
static int check_program(const giql_operand* nodes, int32_t n_nodes, int first, int count, int k, const char* which,
                         bool* uses, const char* owner, bool* can_float);
static int convert_aggs(const giql_pair_expr_agg* aggs, int32_t n_aggs, bool over_pairs, const giql_operand* nodes,
                        int32_t n_nodes, PxaggArgs& xa, bool* any_prog = nullptr, bool* ordered = nullptr) {
  memset(&xa, 0, sizeof(xa));
  MaggArgs& ma = xa.M;
  ma.n_aggs = n_aggs;
  for (int k = 0; k < n_aggs; k++) {
    const giql_pair_expr_agg& g = aggs[k];
    if (g.func < GIQL_AGG_COUNT || g.func > GIQL_AGG_MAX)
      return set_err(GIQL_ERR_INVALID, "aggregate %d: function %d", k, g.func);
    if (g.type < GIQL_T_I32 || g.type > GIQL_T_F64)
      return set_err(GIQL_ERR_INVALID, "aggregate %d: column type %d (int32, int64, float32 or float64)", k, g.type);
    if (!over_pairs && (!g.data || !g.out)) return set_err(GIQL_ERR_INVALID, "aggregate %d: data or out is NULL", k);
    if (!g.out) return set_err(GIQL_ERR_INVALID, "aggregate %d: out is NULL", k);
    if (g.count < 0) return set_err(GIQL_ERR_INVALID, "aggregate %d: a program of %d nodes", k, g.count);
    MaggCol want{g.data, g.valid, g.type};
    PxaggProg prog{0, 0};
    if (g.count > 0) {  // an expression source: checked and typed as giql_hip_eval_expr_dev does it
      if (g.type != GIQL_T_I64 && g.type != GIQL_T_F64)
        return set_err(GIQL_ERR_INVALID, "aggregate %d: result type %d of a program (GIQL_T_I64 or GIQL_T_F64)", k, g.type);
      bool uses[2] = {false, false}, can_float = false;
      GIQL_TRY(check_program(nodes, n_nodes, g.first, g.count, k, "program", uses, "aggregate", &can_float));
      if (can_float && g.type == GIQL_T_I64)
        return set_err(GIQL_ERR_INVALID, "aggregate %d: the program can yield a float, its result type is GIQL_T_I64", k);
      want = MaggCol{nullptr, nullptr, g.type};  // (k_magg_fold reads the type alone)
      prog = PxaggProg{g.first, g.count};
      if (any_prog) *any_prog = true;
    } else if (over_pairs) {
      if (!g.data && g.func != GIQL_AGG_COUNT)
        return set_err(GIQL_ERR_INVALID, "aggregate %d: data is NULL (only COUNT reads validity alone)", k);
      if (g.func == GIQL_AGG_COUNT) want = MaggCol{nullptr, g.valid, MAGG_T_NONE};  // COUNT never reads the values
    }
    int c = 0;
    while (c < ma.n_cols && !(ma.cols[c].data == want.data && ma.cols[c].valid == want.valid && ma.cols[c].type == want.type &&
                              xa.prog[c].first == prog.first && xa.prog[c].count == prog.count)) c++;
    if (c == ma.n_cols) {
      xa.prog[c] = prog;
      ma.cols[ma.n_cols++] = want;
    }
    ma.aggs[k].func = g.func;
    ma.aggs[k].col = c;
    ma.aggs[k].out = (u64*)g.out;
    ma.aggs[k].out_nn = (i64*)g.out_nn;
    if (ordered && g.func != GIQL_AGG_COUNT && (g.type == GIQL_T_F32 || g.type == GIQL_T_F64)) *ordered = true;
  }
  return GIQL_OK;
}

// giql_agg[] as column sources of giql_pair_expr_agg[] (at most MAGG_MAX are copied: the callers check the count)
static const giql_pair_expr_agg* column_sources(const giql_agg* aggs, int32_t n_aggs, giql_pair_expr_agg* out) {
  for (int k = 0; aggs && k < n_aggs && k < MAGG_MAX; k++)
    out[k] = giql_pair_expr_agg{aggs[k].func, aggs[k].type, aggs[k].data, aggs[k].valid, 0, 0, aggs[k].out, aggs[k].out_nn};
  return aggs ? out : nullptr;
}

// The segmented reduction of MERGE's aggregates and of the pair aggregates: per aggregate four carry words per tile of
// MAGG_TILE sorted positions; one launch over the tiles, and a fold of the carries when there is more than one.  The
// launches belong to the caller's Phase.  xa: the programs of a pair aggregate -- k_pxagg_tiles evaluates them at
// (rows_a, rows) and gathers the column sources of the same call; without one it is k_magg_tiles over `rows`.
static size_t magg_sizes(int n_aggs, size_t n) { return (size_t)n_aggs * 4 * cdiv(n, (size_t)MAGG_TILE); }

static void bind_magg(MaggArgs& ma, u64* ws, size_t n) {
  const size_t n_tiles = cdiv(n, (size_t)MAGG_TILE);
  for (int a = 0; a < ma.n_aggs; a++) {
    u64* w = ws + (size_t)a * 4 * n_tiles;
    ma.aggs[a].first_v = w, ma.aggs[a].last_v = w + n_tiles;
    ma.aggs[a].first_c = (i64*)(w + 2 * n_tiles), ma.aggs[a].last_c = (i64*)(w + 3 * n_tiles);
  }
}

static void run_magg(hipStream_t st, const u32* rows, const u32* excl, const u32* flags, u32 n, const MaggArgs& ma,
                     const PxaggArgs* xa = nullptr, const u32* rows_a = nullptr, const DevOperand* nodes = nullptr) {
  const u32 n_tiles = cdiv((u64)n, MAGG_TILE);
  if (xa)
    hipLaunchKernelGGL(k_pxagg_tiles, dim3(n_tiles), dim3(MAGG_TILE), 0, st, rows_a, rows, excl, flags, n, nodes, *xa);
  else
    hipLaunchKernelGGL(k_magg_tiles, dim3(n_tiles), dim3(MAGG_TILE), 0, st, rows, excl, flags, n, ma);
  if (n_tiles > 1)
    hipLaunchKernelGGL(k_magg_fold, dim3(cdiv((u64)n_tiles - 1, 256 / WAVE)), dim3(256), 0, st, excl, flags, n, n_tiles, ma);
}

// ---------------------------------------------------------- CLUSTER / MERGE
// Shared front half: keys + ends on the linear axis, sorted by start, inclusive
// prefix max of the ends, new-cluster flags and their exclusive scan.
struct ClusterBufs {
  LinBufs lb;
  SortBufs sb;
  OsScratch os;
  u32 *pmax = nullptr, *bmax = nullptr, *chrom_lo = nullptr, *flags = nullptr, *excl = nullptr;
  u32* dummy_irr = nullptr;
  u64 *bsums = nullptr, *total = nullptr;
  u32* head_pos = nullptr;
  u32* seg_end = nullptr;  // MERGE under a predicate: MAX(end) per region
  int n_aggs = 0;          // MERGE with aggregates: set before cluster_front
  u64* agg_ws = nullptr;   //   per aggregate the four per-tile carry arrays (merge_agg_kernels.hip.h)
  bool strs = false;       // MERGE with STRING_AGG: set before cluster_front (string_agg_kernels.hip.h)
  u64 *str_g = nullptr, *str_tot = nullptr;  //   G (n + 1), the totals of V and of the region bytes
  u32 *str_v = nullptr, *str_bad = nullptr;  //   V (n + 1), one flag word per string aggregate
};

// MERGE with STRING_AGG: the caller's aggregates (n_bytes is written back) and the order output
struct SaggCall {
  giql_str_agg* strs;
  int n;
  int32_t* out_order;
};

static int cluster_front(giql_hip_ctx* ctx, hipStream_t st, const giql_side* s, int32_t n_chrom,
                         int64_t distance, bool want_rids, bool want_heads, ClusterBufs& cb,
                         const DevPreds* preds = nullptr) {
  const size_t n = (size_t)s->n;
  auto carve = [&](char* base) {
    Carver c{base};
    common_sizes(c, n_chrom, cb.lb);
    sort_sizes(c, n, cb.sb, true, want_rids);
    os_scratch_sizes(c, n, cb.os);
    cb.pmax = c.take<u32>(n);
    cb.bmax = c.take<u32>(cdiv(n, PM_TILE) + 1);
    cb.chrom_lo = c.take<u32>((size_t)n_chrom + 2);
    cb.flags = c.take<u32>(n);
    cb.excl = c.take<u32>(n + 1);
    cb.bsums = c.take<u64>(cdiv((u64)n, SCAN_TILE) + 1);
    cb.total = c.take<u64>(1);
    cb.dummy_irr = c.take<u32>(16);
    cb.head_pos = want_heads ? c.take<u32>(n + 1) : nullptr;
    cb.seg_end = want_heads && preds && preds->n > 0 ? c.take<u32>(n + 1) : nullptr;
    cb.agg_ws = cb.n_aggs ? c.take<u64>(magg_sizes(cb.n_aggs, n)) : nullptr;
    cb.str_g = cb.strs ? c.take<u64>(n + 1) : nullptr;
    cb.str_v = cb.strs ? c.take<u32>(n + 1) : nullptr;
    cb.str_tot = cb.strs ? c.take<u64>(2) : nullptr;
    cb.str_bad = cb.strs ? c.take<u32>(SAGG_MAX) : nullptr;
    return c.off;
  };
  GIQL_TRY(claim_arena(ctx, st, carve));
  giql_side none;
  memset(&none, 0, sizeof(none));
  GIQL_TRY(run_spans(ctx, st, *s, none, n_chrom, cb.lb));
  GIQL_TRY(run_linearize(ctx, st, *s, n_chrom, cb.lb, Side::A, LinTarget::keys_ends(cb.sb.key[0], cb.sb.end[0], cb.dummy_irr),
                         LinOptions().keeping_irregular().counting_starts(cb.os.starts())));
  {
    Phase ph(ctx, st, GIQL_PH_AUX);
    hipLaunchKernelGGL(k_check_not_inverted, dim3(cdiv(n, 256)), dim3(256), 0, st, view_of(*s),
                       ctx->d_meta);
  }
  GIQL_TRY(run_sort_onesweep(ctx, st, cb.sb, sort_by_start(cb.os, n)));
  GIQL_TRY(run_pmax(ctx, st, cb.sb.end[0], (u32)n, cb.pmax, cb.bmax));
  HIP_TRY(hipMemsetAsync(cb.flags, 0, n * sizeof(u32), st));
  {
    Phase ph(ctx, st, GIQL_PH_COUNT, 3);
    hipLaunchKernelGGL(k_chrom_bounds, dim3(cdiv((u64)n_chrom + 1, 256)), dim3(256), 0, st,
                       cb.lb.chrom_first, n_chrom, cb.sb.key[0], (u32)n, cb.chrom_lo);
    hipLaunchKernelGGL(k_cluster_firsts, dim3(cdiv((u64)n_chrom, 256)), dim3(256), 0, st, cb.chrom_lo,
                       n_chrom, (u32)n, cb.flags);
    hipLaunchKernelGGL(k_cluster_flags, dim3(cdiv(n, 256)), dim3(256), 0, st, cb.sb.key[0], cb.pmax,
                       (u32)n, (u64)(distance > 0 ? distance : 0), cb.flags);
    if (preds && preds->n > 0)  // (needs the row ids: want_rids)
      hipLaunchKernelGGL(k_cluster_pred_flags, dim3(cdiv(n, 256)), dim3(256), 0, st, cb.sb.rid[0], (u32)n, *preds,
                         cb.flags);
    GIQL_TRY(post_launch("cluster flags"));
  }
  GIQL_TRY(run_scan<u32>(ctx, st, GIQL_PH_SCAN, cb.flags, (u64)n, cb.excl, cb.bsums, cb.total));
  return GIQL_OK;
}

static int check_cluster_args(giql_hip_ctx* ctx, const giql_side* s, int32_t n_chrom) {
  if (!ctx) return set_err(GIQL_ERR_INVALID, "ctx is NULL");
  GIQL_TRY(check_side(s, "s"));
  if (n_chrom < 0) return set_err(GIQL_ERR_INVALID, "n_chrom < 0");
  if (s->start_off != 0 || s->end_off != 0)
    return set_err(GIQL_ERR_INVALID,
                   "CLUSTER / MERGE read the raw start / end columns (cluster.py:246-263): offsets must be 0");
  if ((size_t)s->n > OS_MAX_ROWS) return set_err(GIQL_ERR_INVALID, "side larger than 2^30 rows");
  return GIQL_OK;
}

static int cluster_status(giql_hip_ctx* ctx, hipStream_t st) {
  HIP_TRY(hipMemcpyAsync(ctx->h_meta, ctx->d_meta, sizeof(DevMeta), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (ctx->h_meta->status == -1)
    return set_err(GIQL_ERR_INVALID, "CLUSTER / MERGE need start <= end on every row");
  return read_meta(ctx, st);
}

static int giql_hip_cluster_dev_impl(giql_hip_ctx* ctx, const giql_side* s, int32_t n_chrom, int64_t distance,
                         int64_t* cluster_id_out, void* stream, const DevPreds* preds = nullptr) {
  GIQL_TRY(check_cluster_args(ctx, s, n_chrom));
  GIQL_TRY(begin_call(ctx, s->n));
  hipStream_t st = (hipStream_t)stream;
  if (s->n == 0) return GIQL_OK;
  if (!cluster_id_out) return set_err(GIQL_ERR_INVALID, "cluster_id_out is NULL");
  if (n_chrom == 0) return set_err(GIQL_ERR_CHROM, "rows but n_chrom = 0");
  ClusterBufs cb;
  GIQL_TRY(cluster_front(ctx, st, s, n_chrom, distance, true, false, cb, preds));
  {
    Phase ph(ctx, st, GIQL_PH_FILL);
    hipLaunchKernelGGL(k_cluster_ids, dim3(cdiv((u64)s->n, 256)), dim3(256), 0, st, cb.sb.key[0],
                       cb.sb.rid[0], cb.flags, cb.excl, (u32)s->n, cb.lb.chrom_first, n_chrom,
                       cb.chrom_lo, (i64*)cluster_id_out);
    GIQL_TRY(post_launch("cluster ids"));
  }
  GIQL_TRY(cluster_status(ctx, st));
  collect_spans(ctx);
  ctx->stats.n_out = s->n;
  ctx->stats.span = (int64_t)ctx->h_meta->total_span;
  return GIQL_OK;
}

int giql_hip_cluster_dev(giql_hip_ctx* ctx, const giql_side* s, int32_t n_chrom, int64_t distance,
                         int64_t* cluster_id_out, void* stream) {
  return with_order_fallback(ctx, [&] { return giql_hip_cluster_dev_impl(ctx, s, n_chrom, distance, cluster_id_out, stream); });
}

static int check_operand(const giql_operand& o, int k, const char* which, const char* owner = "predicate");

// giql_pred[] -> the by-value kernel argument; uses[side] = a column of that side is read
// A well-formed postfix program: every operator finds its arguments, one value is left, the stack stays within
// SEL_X_STACK.  uses[side] as in convert_preds.  `owner` k `which` names the program in a message ("predicate 2 lhs",
// "output 0 program").
// can_float (giql_hip_eval_expr_dev): the static type of the result -- per stack slot, can the value be a float?  A
// float leaf is an F32 / F64 column or a float literal, `/` yields a float, arithmetic / NEG / ABS / LEAST / GREATEST
// the OR of their arguments, IF `then OR else`; comparisons, IS [NOT] NULL, AND / OR / NOT and NULL are integers.
static int check_program(const giql_operand* nodes, int32_t n_nodes, int first, int count, int k, const char* which,
                         bool* uses, const char* owner = "predicate", bool* can_float = nullptr) {
  if (!nodes || first < 0 || count < 1 || first > n_nodes - count)
    return set_err(GIQL_ERR_INVALID, "%s %d %s: expression nodes [%d, %lld) outside the %d given", owner, k, which, first,
                   (long long)first + count, n_nodes);
  int sp = 0;
  bool fl[SEL_X_STACK + 1];
  for (int t = first; t < first + count; t++) {
    const giql_operand& nd = nodes[t];
    if (nd.side == GIQL_SIDE_A || nd.side == GIQL_SIDE_B || nd.side == GIQL_SIDE_LIT || nd.side == GIQL_X_NULL) {
      if (nd.side != GIQL_X_NULL) GIQL_TRY(check_operand(nd, k, which, owner));
      if (uses && (nd.side == GIQL_SIDE_A || nd.side == GIQL_SIDE_B)) uses[nd.side] = true;
      if (++sp > SEL_X_STACK) return set_err(GIQL_ERR_INVALID, "%s %d %s: expression deeper than %d", owner, k, which, SEL_X_STACK);
      fl[sp - 1] = nd.side == GIQL_SIDE_LIT ? nd.lit_is_float != 0
                                            : (nd.side != GIQL_X_NULL && (nd.type == GIQL_T_F32 || nd.type == GIQL_T_F64));
    } else if (nd.side == GIQL_X_NEG || nd.side == GIQL_X_ABS || nd.side == GIQL_X_ISNULL || nd.side == GIQL_X_NOTNULL ||
               nd.side == GIQL_X_NOT) {
      if (sp < 1) return set_err(GIQL_ERR_INVALID, "%s %d %s: malformed expression", owner, k, which);
      if (nd.side != GIQL_X_NEG && nd.side != GIQL_X_ABS) fl[sp - 1] = false;
    } else if ((nd.side >= GIQL_X_ADD && nd.side <= GIQL_X_GREATEST) || (nd.side >= GIQL_X_EQ && nd.side <= GIQL_X_GE) ||
               nd.side == GIQL_X_AND || nd.side == GIQL_X_OR) {
      if (sp < 2) return set_err(GIQL_ERR_INVALID, "%s %d %s: malformed expression", owner, k, which);
      sp--;
      fl[sp - 1] = nd.side == GIQL_X_DIV || (nd.side <= GIQL_X_GREATEST && (fl[sp - 1] || fl[sp]));
    } else if (nd.side == GIQL_X_IF) {
      if (sp < 3) return set_err(GIQL_ERR_INVALID, "%s %d %s: malformed expression (IF needs three values)", owner, k, which);
      sp -= 2;
      fl[sp - 1] = fl[sp] || fl[sp + 1];
    } else {
      return set_err(GIQL_ERR_INVALID, "%s %d %s: expression node kind %d", owner, k, which, nd.side);
    }
  }
  if (sp != 1) return set_err(GIQL_ERR_INVALID, "%s %d %s: malformed expression", owner, k, which);
  if (can_float) *can_float = fl[0];
  return GIQL_OK;
}

static int convert_preds(const giql_pred* preds, int32_t n_preds, DevPreds& ps, bool* uses,
                         const giql_operand* nodes = nullptr, int32_t n_nodes = 0, bool* any_expr = nullptr) {
  static_assert(sizeof(giql_operand) == sizeof(DevOperand), "giql_operand layout");
  static_assert(sizeof(giql_pred) == sizeof(DevPred), "giql_pred layout");
  memset(&ps, 0, sizeof(ps));
  ps.n = n_preds;
  for (int k = 0; k < n_preds; k++) {
    const bool unary = preds[k].op == GIQL_OP_IS_NULL || preds[k].op == GIQL_OP_NOT_NULL || preds[k].op == GIQL_OP_IS_TRUE;
    if (preds[k].op < GIQL_OP_EQ || preds[k].op > GIQL_OP_IS_TRUE)
      return set_err(GIQL_ERR_INVALID, "predicate %d: operator %d", k, preds[k].op);
    if (preds[k].group < 0) return set_err(GIQL_ERR_INVALID, "predicate %d: group %d", k, preds[k].group);
    for (int w = 0; w < (unary ? 1 : 2); w++) {
      const giql_operand& o = w ? preds[k].rhs : preds[k].lhs;
      if (o.side == GIQL_SIDE_EXPR) {
        GIQL_TRY(check_program(nodes, n_nodes, (int)o.lit_i, o.type, k, w ? "rhs" : "lhs", uses));
        if (any_expr) *any_expr = true;
      } else {
        GIQL_TRY(check_operand(o, k, w ? "rhs" : "lhs"));
        if (uses && o.side != GIQL_SIDE_LIT) uses[o.side] = true;
      }
    }
    memcpy(&ps.p[k], &preds[k], sizeof(DevPred));
    if (unary) {  // the right operand is not read: make it a harmless literal
      memset(&ps.p[k].rhs, 0, sizeof(DevOperand));
      ps.p[k].rhs.side = GIQL_SIDE_LIT;
    }
  }
  return GIQL_OK;
}

int giql_hip_cluster_pred_dev(giql_hip_ctx* ctx, const giql_side* s, int32_t n_chrom, int64_t distance,
                              const giql_pred* preds, int32_t n_preds, int64_t* cluster_id_out, void* stream) {
  if (n_preds < 0 || n_preds > SEL_MAX_PREDS || (n_preds && !preds))
    return set_err(GIQL_ERR_INVALID, "bad predicates (at most %d)", SEL_MAX_PREDS);
  DevPreds ps;
  GIQL_TRY(convert_preds(preds, n_preds, ps, nullptr));
  return with_order_fallback(ctx, [&] { return giql_hip_cluster_dev_impl(ctx, s, n_chrom, distance, cluster_id_out, stream, &ps); });
}

static int giql_hip_merge_dev_impl(giql_hip_ctx* ctx, const giql_side* s, int32_t n_chrom, int64_t distance,
                       int32_t* out_chrom, int32_t* out_start, int32_t* out_end,
                       int64_t* out_count, int64_t capacity, int64_t* n_out, void* stream,
                       const DevPreds* preds = nullptr, MaggArgs* aggs = nullptr, const SaggCall* sc = nullptr) {
  GIQL_TRY(check_cluster_args(ctx, s, n_chrom));
  if (!n_out) return set_err(GIQL_ERR_INVALID, "n_out is NULL");
  GIQL_TRY(begin_call(ctx, s->n));
  hipStream_t st = (hipStream_t)stream;
  *n_out = 0;
  if (s->n == 0) {
    for (int a = 0; sc && a < sc->n; a++) {  // no region: the offsets of an empty string column
      sc->strs[a].n_bytes = 0;
      if (sc->strs[a].out_offsets) HIP_TRY(hipMemsetAsync(sc->strs[a].out_offsets, 0, sizeof(int32_t), st));
    }
    if (sc) HIP_TRY(hipStreamSynchronize(st));
    return GIQL_OK;
  }
  if (!out_chrom || !out_start || !out_end) return set_err(GIQL_ERR_INVALID, "output buffer is NULL");
  if (n_chrom == 0) return set_err(GIQL_ERR_CHROM, "rows but n_chrom = 0");
  ClusterBufs cb;
  const bool pred = preds && preds->n > 0;
  cb.n_aggs = aggs ? aggs->n_aggs : 0;
  cb.strs = sc != nullptr;
  GIQL_TRY(cluster_front(ctx, st, s, n_chrom, distance, pred || aggs || sc, true, cb, preds));
  u64 h_total = 0;
  HIP_TRY(hipMemcpyAsync(&h_total, cb.total, sizeof(u64), hipMemcpyDeviceToHost, st));
  GIQL_TRY(cluster_status(ctx, st));
  if ((int64_t)h_total > capacity)
    return set_err(GIQL_ERR_CAPACITY, "%llu merged regions, capacity %lld",
                   (unsigned long long)h_total, (long long)capacity);
  {
    Phase ph(ctx, st, GIQL_PH_FILL, (pred ? 3 : 2) + (aggs ? 2 : 0));
    hipLaunchKernelGGL(k_merge_heads, dim3(cdiv((u64)s->n, 256)), dim3(256), 0, st, cb.flags, cb.excl,
                       (u32)s->n, cb.head_pos);
    if (pred && h_total) {
      HIP_TRY(hipMemsetAsync(cb.seg_end, 0, (size_t)h_total * sizeof(u32), st));
      hipLaunchKernelGGL(k_merge_segmax, dim3(cdiv((u64)s->n, 256)), dim3(256), 0, st, cb.sb.end[0], cb.excl,
                         cb.flags, (u32)s->n, cb.seg_end);
    }
    if (h_total)
      hipLaunchKernelGGL(k_merge_rows, dim3(cdiv(h_total, 256)), dim3(256), 0, st, cb.head_pos,
                         (u32)h_total, (u32)s->n, cb.sb.key[0], cb.pmax, pred ? cb.seg_end : (u32*)nullptr, cb.lb.chrom_first,
                         cb.lb.chrom_base, n_chrom, out_chrom, out_start, out_end, (i64*)out_count);
    if (aggs && h_total) {  // one segmented reduction over the sorted order; every region gets exactly one writer
      bind_magg(*aggs, cb.agg_ws, (size_t)s->n);
      run_magg(st, cb.sb.rid[0], cb.excl, cb.flags, (u32)s->n, *aggs);
    }
    GIQL_TRY(post_launch("merge rows"));
  }
  u64 str_total[SAGG_MAX] = {0, 0, 0, 0};
  u32 str_bad[SAGG_MAX] = {0, 0, 0, 0};
  if (sc) {
    // The sort is done: its second buffers are free, and hold the per-position lengths, flags and the region bytes.
    const u32 n = (u32)s->n, m = (u32)h_total;  // (m >= 1: the first row is a head)
    u32 *c = cb.sb.key[1], *v = cb.sb.end[1], *rb = cb.sb.rid[1];
    HIP_TRY(hipMemsetAsync(cb.str_bad, 0, SAGG_MAX * sizeof(u32), st));
    for (int a = 0; a < sc->n; a++) {
      const giql_str_agg& g = sc->strs[a];
      {
        Phase ph(ctx, st, GIQL_PH_COUNT, 1);
        hipLaunchKernelGGL(k_sagg_len, dim3(cdiv((u64)n, SAGG_NT)), dim3(SAGG_NT), 0, st, cb.sb.rid[0], n, g.offsets,
                           g.valid, (u32)g.sep_len, c, v, a == 0 ? sc->out_order : (int32_t*)nullptr, cb.str_bad + a);
        GIQL_TRY(post_launch("string_agg lengths"));
      }
      GIQL_TRY(run_scan<u64>(ctx, st, GIQL_PH_SCAN, c, (u64)n, cb.str_g, cb.bsums, cb.str_g + n));
      GIQL_TRY(run_scan<u32>(ctx, st, GIQL_PH_SCAN, v, (u64)n, cb.str_v, cb.bsums, cb.str_tot));
      {
        Phase ph(ctx, st, GIQL_PH_FILL, 1);
        hipLaunchKernelGGL(k_sagg_regions, dim3(cdiv((u64)m, SAGG_NT)), dim3(SAGG_NT), 0, st, cb.head_pos, m, n,
                           cb.str_g, cb.str_v, cb.str_tot, (u32)g.sep_len, rb, (i64*)g.out_nn);
        GIQL_TRY(post_launch("string_agg regions"));
      }
      GIQL_TRY(run_scan<u32>(ctx, st, GIQL_PH_SCAN, rb, (u64)m, rb, cb.bsums, cb.str_tot + 1));
      {
        Phase ph(ctx, st, GIQL_PH_FILL, 1);
        hipLaunchKernelGGL(k_sagg_rows, dim3(cdiv((u64)n, SAGG_NT)), dim3(SAGG_NT), 0, st, cb.excl, cb.flags, cb.head_pos,
                           n, m, cb.str_g, cb.str_v, v, rb, cb.str_tot + 1, g.out_offsets, g.row_dst);
        GIQL_TRY(post_launch("string_agg rows"));
      }
      // (a pageable destination: the copy has landed when the call returns, before the next aggregate's scan)
      HIP_TRY(hipMemcpyAsync(&str_total[a], cb.str_tot + 1, sizeof(u64), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
    }
    HIP_TRY(hipMemcpyAsync(str_bad, cb.str_bad, sizeof(str_bad), hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  collect_spans(ctx);
  *n_out = (int64_t)h_total;
  for (int a = 0; sc && a < sc->n; a++)
    if (str_bad[a])
      return set_err(GIQL_ERR_INVALID, "string aggregate %d: an offset pair is negative or decreases", a);
  int over = -1;
  for (int a = 0; sc && a < sc->n; a++) {
    const bool fits = str_total[a] < 0x7FFFFFFFull || (str_total[a] == 0x7FFFFFFFull && sc->strs[a].sep_len == 0);
    sc->strs[a].n_bytes = fits ? (int64_t)str_total[a] : -1;
    if (!fits && over < 0) over = a;
  }
  if (over >= 0)
    return set_err(GIQL_ERR_CAPACITY, "string aggregate %d: output of %llu bytes or more exceeds int32 offsets", over,
                   (unsigned long long)str_total[over]);  // (a single region past the limit was counted as 2^31 bytes)
  ctx->stats.n_out = (int64_t)h_total;
  ctx->stats.span = (int64_t)ctx->h_meta->total_span;
  return GIQL_OK;
}

int giql_hip_merge_dev(giql_hip_ctx* ctx, const giql_side* s, int32_t n_chrom, int64_t distance,
                       int32_t* out_chrom, int32_t* out_start, int32_t* out_end, int64_t* out_count,
                       int64_t capacity, int64_t* n_out, void* stream) {
  return with_order_fallback(ctx, [&] { return giql_hip_merge_dev_impl(ctx, s, n_chrom, distance, out_chrom, out_start, out_end, out_count, capacity, n_out, stream); });
}

int giql_hip_merge_pred_dev(giql_hip_ctx* ctx, const giql_side* s, int32_t n_chrom, int64_t distance,
                            const giql_pred* preds, int32_t n_preds, int32_t* out_chrom, int32_t* out_start,
                            int32_t* out_end, int64_t* out_count, int64_t capacity, int64_t* n_out, void* stream) {
  if (n_preds < 0 || n_preds > SEL_MAX_PREDS || (n_preds && !preds))
    return set_err(GIQL_ERR_INVALID, "bad predicates (at most %d)", SEL_MAX_PREDS);
  DevPreds ps;
  GIQL_TRY(convert_preds(preds, n_preds, ps, nullptr));
  return with_order_fallback(ctx, [&] { return giql_hip_merge_dev_impl(ctx, s, n_chrom, distance, out_chrom, out_start, out_end, out_count, capacity, n_out, stream, &ps); });
}

int giql_hip_merge_agg_dev(giql_hip_ctx* ctx, const giql_side* s, int32_t n_chrom, int64_t distance,
                           const giql_pred* preds, int32_t n_preds, const giql_agg* aggs, int32_t n_aggs,
                           int32_t* out_chrom, int32_t* out_start, int32_t* out_end, int64_t* out_count,
                           int64_t capacity, int64_t* n_out, void* stream) {
  if (n_preds < 0 || n_preds > SEL_MAX_PREDS || (n_preds && !preds))
    return set_err(GIQL_ERR_INVALID, "bad predicates (at most %d)", SEL_MAX_PREDS);
  if (n_aggs < 1 || n_aggs > MAGG_MAX || !aggs)
    return set_err(GIQL_ERR_INVALID, "%d aggregates: MERGE takes 1 to %d", n_aggs, MAGG_MAX);
  giql_pair_expr_agg cols[MAGG_MAX];
  PxaggArgs xa;
  GIQL_TRY(convert_aggs(column_sources(aggs, n_aggs, cols), n_aggs, false, nullptr, 0, xa));
  DevPreds ps;
  GIQL_TRY(convert_preds(preds, n_preds, ps, nullptr));
  return with_order_fallback(ctx, [&] { return giql_hip_merge_dev_impl(ctx, s, n_chrom, distance, out_chrom, out_start, out_end, out_count, capacity, n_out, stream, &ps, &xa.M); });
}

// MERGE with STRING_AGG (include/giql_hip_string_agg.h): giql_hip_merge_agg_dev with 0..8 numeric aggregates plus the
// plan of 1..4 string aggregates; giql_hip_concat_utf8_fill_dev writes their bytes.  The caller owns every array the
// fill reads: the pair keeps no plan in the context.
int giql_hip_merge_str_dev(giql_hip_ctx* ctx, const giql_side* s, int32_t n_chrom, int64_t distance,
                           const giql_pred* preds, int32_t n_preds, const giql_agg* aggs, int32_t n_aggs,
                           giql_str_agg* strs, int32_t n_strs, int32_t* out_chrom, int32_t* out_start,
                           int32_t* out_end, int64_t* out_count, int32_t* out_order, int64_t capacity, int64_t* n_out,
                           void* stream) {
  if (n_preds < 0 || n_preds > SEL_MAX_PREDS || (n_preds && !preds))
    return set_err(GIQL_ERR_INVALID, "bad predicates (at most %d)", SEL_MAX_PREDS);
  if (n_aggs < 0 || n_aggs > MAGG_MAX || (n_aggs && !aggs))
    return set_err(GIQL_ERR_INVALID, "%d aggregates: MERGE with STRING_AGG takes 0 to %d", n_aggs, MAGG_MAX);
  if (n_strs < 1 || n_strs > SAGG_MAX || !strs)
    return set_err(GIQL_ERR_INVALID, "%d string aggregates: MERGE takes 1 to %d", n_strs, SAGG_MAX);
  const bool rows = s && s->n > 0;
  for (int k = 0; k < n_strs; k++) {
    if (strs[k].sep_len < 0 || strs[k].sep_len > SAGG_SEP_MAX)
      return set_err(GIQL_ERR_INVALID, "string aggregate %d: separator of %d bytes (0 to %d)", k, strs[k].sep_len,
                     SAGG_SEP_MAX);
    if (rows && (!strs[k].offsets || !strs[k].out_offsets || !strs[k].out_nn || !strs[k].row_dst))
      return set_err(GIQL_ERR_INVALID, "string aggregate %d: offsets, out_offsets, out_nn or row_dst is NULL", k);
  }
  if (rows && !out_order) return set_err(GIQL_ERR_INVALID, "out_order is NULL");
  giql_pair_expr_agg cols[MAGG_MAX];
  PxaggArgs xa;
  GIQL_TRY(convert_aggs(column_sources(aggs, n_aggs, cols), n_aggs, false, nullptr, 0, xa));
  DevPreds ps;
  GIQL_TRY(convert_preds(preds, n_preds, ps, nullptr));
  const SaggCall sc{strs, n_strs, out_order};
  return with_order_fallback(ctx, [&] { return giql_hip_merge_dev_impl(ctx, s, n_chrom, distance, out_chrom, out_start, out_end, out_count, capacity, n_out, stream, &ps, n_aggs ? &xa.M : nullptr, &sc); });
}

int giql_hip_concat_utf8_fill_dev(giql_hip_ctx* ctx, const int32_t* offsets, const uint8_t* data, int64_t n_rows,
                                  const int32_t* order, const uint32_t* row_dst, int64_t n, const uint8_t* sep,
                                  int32_t sep_len, uint8_t* out_data, void* stream) {
  if (!ctx || n < 0 || n > 0x7FFFFFF0ll || n_rows < 0 || n_rows > 0x7FFFFFFFll)
    return set_err(GIQL_ERR_INVALID, "bad arguments");
  if (sep_len < 0 || sep_len > SAGG_SEP_MAX || (sep_len && !sep))
    return set_err(GIQL_ERR_INVALID, "separator of %d bytes (0 to %d, not NULL)", sep_len, SAGG_SEP_MAX);
  if (n == 0) return GIQL_OK;
  if (!order || !row_dst || (n_rows > 0 && !offsets)) return set_err(GIQL_ERR_INVALID, "NULL buffer");
  GIQL_TRY(begin_call_beside_plan(ctx));
  hipStream_t st = (hipStream_t)stream;
  SaggSep sp;
  memset(&sp, 0, sizeof(sp));
  sp.len = (u32)sep_len;
  if (sep_len) memcpy(sp.b, sep, (size_t)sep_len);
  GIQL_TRY(begin_status(ctx, st));
  u32 grid = cdiv((u64)n, (u64)SAGG_NT * 2);
  if (grid > 2u * GIQL_STREAM_GRID) grid = 2u * GIQL_STREAM_GRID;
  {
    Phase ph(ctx, st, GIQL_PH_AUX);
    hipLaunchKernelGGL(k_sagg_fill, dim3(grid), dim3(SAGG_NT), 0, st, offsets, data, (u32)n_rows, order, row_dst, (u64)n,
                       sp, out_data, &ctx->d_meta->status);
    GIQL_TRY(post_launch("concat_utf8_fill"));
  }
  int status;
  GIQL_TRY(finish_status(ctx, st, status));
  if (status != 0)
    return set_err(GIQL_ERR_INVALID, "concat_utf8_fill: a row id outside the column, a decreasing offset pair or a "
                                     "separator before the output's start");
  ctx->stats.n_out = n;
  return GIQL_OK;
}

// ------------------------------------------------ aggregates over a join's pairs, per left row
// include/giql_hip_pair_agg.h.  A post-pass over the caller's pair arrays (pair_agg_kernels.hip.h): check + load ->
// stable sort by row_b (only where a float SUM / MIN / MAX makes the order matter) -> stable sort by row_a -> region flags ->
// scan -> k_magg_tiles / k_magg_fold over the regions -> scatter to the A rows.  The sorts are run_sort with as many
// passes as the ids have digits: the same launches on every context, whatever its sort switches say.
static int pagg_digits(int64_t n_rows) {
  int p = 0;
  while (p < 4 && ((u64)(n_rows > 0 ? n_rows - 1 : 0) >> (8 * p)) != 0) p++;
  return p;
}

// One pipeline for both entry points: an aggregate's value source is a column of B (count == 0) or a program over the
// staged nodes (include/giql_hip_pair_expr_agg.h).  Without a program the reduction is k_magg_tiles, as it was before
// programs existed; with one it is k_pxagg_tiles, which also gathers the column sources of the same call.
static int pair_agg_impl(giql_hip_ctx* ctx, const int32_t* row_a, const int32_t* row_b, int64_t n_pairs, int64_t n_a,
                         int64_t n_b, const giql_operand* nodes, int32_t n_nodes, const giql_pair_expr_agg* aggs,
                         int32_t n_aggs, int64_t* pairs_out, void* stream) {
  if (!ctx) return set_err(GIQL_ERR_INVALID, "ctx is NULL");
  // Begins a call before its own checks: whatever it goes on to return, a plan the context held is gone.
  GIQL_TRY(begin_call(ctx, n_a, n_b));
  if (n_pairs < 0 || n_a < 0 || n_b < 0 || n_a > 0x7FFFFFFFll || n_b > 0x7FFFFFFFll)
    return set_err(GIQL_ERR_INVALID, "bad arguments (n_pairs, n_a, n_b: 0 to 2^31 - 1)");
  if (n_pairs >= ((int64_t)1 << 31))
    return set_err(GIQL_ERR_INVALID, "%lld pairs: one call aggregates fewer than 2^31", (long long)n_pairs);
  if (n_aggs < 0 || n_aggs > MAGG_MAX || (n_aggs && !aggs))
    return set_err(GIQL_ERR_INVALID, "%d aggregates: a pair aggregate takes 0 to %d", n_aggs, MAGG_MAX);
  if (n_nodes < 0 || n_nodes > SEL_MAX_NODES || (n_nodes && !nodes))
    return set_err(GIQL_ERR_INVALID, "%d expression nodes: a pair aggregate takes 0 to %d", n_nodes, SEL_MAX_NODES);
  PxaggArgs xa;
  MaggArgs& ma = xa.M;
  bool any_prog = false, ordered = false;
  GIQL_TRY(convert_aggs(aggs, n_aggs, true, nodes, n_nodes, xa, &any_prog, &ordered));
  if (n_a > 0 && !pairs_out) return set_err(GIQL_ERR_INVALID, "pairs_out is NULL");
  if (n_a > 0 && n_pairs > 0 && (!row_a || !row_b)) return set_err(GIQL_ERR_INVALID, "row_a or row_b is NULL");
  if (n_a == 0) return GIQL_OK;
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(pairs_out, 0, (size_t)n_a * sizeof(int64_t), st));
  for (int k = 0; k < n_aggs; k++) {
    HIP_TRY(hipMemsetAsync(aggs[k].out, 0, (size_t)n_a * sizeof(u64), st));
    if (aggs[k].out_nn) HIP_TRY(hipMemsetAsync(aggs[k].out_nn, 0, (size_t)n_a * sizeof(i64), st));
  }
  if (n_pairs == 0) {
    HIP_TRY(hipStreamSynchronize(st));
    return GIQL_OK;
  }
  if (n_b == 0) return set_err(GIQL_ERR_INVALID, "pair aggregate: pairs over a B table without rows");
  const size_t n = (size_t)n_pairs;
  const size_t m_max = n < (size_t)n_a ? n : (size_t)n_a;  // regions: distinct A rows among the pairs
  const u32 n_tiles = cdiv(n, MAGG_TILE), rs_tiles = cdiv(n, RS_TILE);
  SortBufs sb;
  u32 *tile_hist = nullptr, *flags = nullptr, *excl = nullptr, *head_pos = nullptr;
  u64 *bsums = nullptr, *total = nullptr, *seg = nullptr, *carry = nullptr;
  DevOperand* d_nodes = nullptr;
  auto carve = [&](char* base) {
    Carver c{base};
    sort_sizes_key_payload(c, n, sb);  // 16 bytes per pair: (row_b, row_a) twice -- no row id column, nothing reads one
    tile_hist = c.take<u32>((size_t)rs_tiles * RS_BINS);
    const size_t scan_max = (size_t)rs_tiles * RS_BINS > n ? (size_t)rs_tiles * RS_BINS : n;
    bsums = c.take<u64>(cdiv(scan_max, SCAN_TILE) + 2);
    total = c.take<u64>(1);
    flags = c.take<u32>(n);
    excl = c.take<u32>(n + 1);
    head_pos = c.take<u32>(m_max + 1);
    seg = c.take<u64>((size_t)n_aggs * 2 * m_max);
    carry = c.take<u64>(magg_sizes(n_aggs, n));
    if (any_prog) d_nodes = c.take<DevOperand>(SEL_MAX_NODES);
    return c.off;
  };
  GIQL_TRY(claim_arena(ctx, st, carve));
  GIQL_TRY(begin_status(ctx, st));
  // (pageable source: staged by the runtime before the call returns)
  if (any_prog) HIP_TRY(hipMemcpyAsync(d_nodes, nodes, (size_t)n_nodes * sizeof(DevOperand), hipMemcpyHostToDevice, st));
  const u32 grid = cdiv(n, PAGG_NT);
  {
    Phase ph(ctx, st, GIQL_PH_AUX);
    hipLaunchKernelGGL(k_pagg_load, dim3(grid), dim3(PAGG_NT), 0, st, row_a, row_b, (u32)n, (u32)n_a, (u32)n_b,
                       sb.key[0], sb.end[0], &ctx->d_meta->status);
    GIQL_TRY(post_launch("pair aggregate (load)"));
  }
  if (ordered) GIQL_TRY(run_sort(ctx, st, sb, (u32)n, tile_hist, bsums, pagg_digits(n_b)));
  SortBufs by_a = sb.keyed_by_end();  // (taken after the first sort: a view does not follow a flip)
  GIQL_TRY(run_sort(ctx, st, by_a, (u32)n, tile_hist, bsums, pagg_digits(n_a)));
  const u32 *sorted_a = by_a.key[0], *sorted_b = by_a.end[0];
  {
    Phase ph(ctx, st, GIQL_PH_COUNT);
    hipLaunchKernelGGL(k_pagg_heads, dim3(grid), dim3(PAGG_NT), 0, st, sorted_a, (u32)n, flags);
    GIQL_TRY(post_launch("pair aggregate (heads)"));
  }
  GIQL_TRY(run_scan<u32>(ctx, st, GIQL_PH_SCAN, flags, (u64)n, excl, bsums, total));
  PaggScatter sc;
  memset(&sc, 0, sizeof(sc));
  sc.n_aggs = n_aggs;
  for (int k = 0; k < n_aggs; k++) {  // the reduction writes per region, the scatter carries that to the A rows
    u64* sv = seg + (size_t)k * 2 * m_max;
    ma.aggs[k].out = sv, ma.aggs[k].out_nn = (i64*)(sv + m_max);
    sc.a[k] = PaggOut{sv, (const i64*)(sv + m_max), (u64*)aggs[k].out, (i64*)aggs[k].out_nn};
  }
  bind_magg(ma, carry, n);
  {
    Phase ph(ctx, st, GIQL_PH_FILL, 2 + (n_aggs ? (n_tiles > 1 ? 2 : 1) : 0));
    hipLaunchKernelGGL(k_merge_heads, dim3(grid), dim3(256), 0, st, flags, excl, (u32)n, head_pos);
    if (n_aggs) run_magg(st, sorted_b, excl, flags, (u32)n, ma, any_prog ? &xa : nullptr, sorted_a, d_nodes);
    hipLaunchKernelGGL(k_pagg_scatter, dim3(grid), dim3(PAGG_NT), 0, st, sorted_a, flags, excl, head_pos, total, (u32)n,
                       (u32)n_a, (i64*)pairs_out, sc);
    GIQL_TRY(post_launch("pair aggregate"));
  }
  int status;
  GIQL_TRY(finish_status(ctx, st, status));
  if (status != 0)
    return set_err(GIQL_ERR_INVALID, "pair aggregate: a row_a outside [0, %lld) or a row_b outside [0, %lld)",
                   (long long)n_a, (long long)n_b);
  ctx->stats.n_out = n_a;
  return GIQL_OK;
}

int giql_hip_pair_agg_dev(giql_hip_ctx* ctx, const int32_t* row_a, const int32_t* row_b, int64_t n_pairs, int64_t n_a,
                          int64_t n_b, const giql_agg* aggs, int32_t n_aggs, int64_t* pairs_out, void* stream) {
  giql_pair_expr_agg cols[MAGG_MAX];
  return pair_agg_impl(ctx, row_a, row_b, n_pairs, n_a, n_b, nullptr, 0, column_sources(aggs, n_aggs, cols), n_aggs, pairs_out, stream);
}

int giql_hip_pair_expr_agg_dev(giql_hip_ctx* ctx, const int32_t* row_a, const int32_t* row_b, int64_t n_pairs,
                               int64_t n_a, int64_t n_b, const giql_operand* nodes, int32_t n_nodes,
                               const giql_pair_expr_agg* aggs, int32_t n_aggs, int64_t* pairs_out, void* stream) {
  return pair_agg_impl(ctx, row_a, row_b, n_pairs, n_a, n_b, nodes, n_nodes, aggs, n_aggs, pairs_out, stream);
}

// ----------------------------------------------------------------- DISJOIN
// Count-then-fill, like the INNER pair.  Stages (disjoin_kernels.hip.h): spans of both sides on one axis ->
// the reference's 2n event keys -> ONE (key, id) sort -> breakpoints + coverage through two scans -> per-target
// counts in input order -> int64 offsets; the fill is output-major.
struct DisjoinBufs : EventBufs {
  u32 *bp = nullptr, *cov = nullptr, *ncov = nullptr, *cbp = nullptr, *cnt = nullptr, *lo_first = nullptr;
  u64 *off = nullptr, *total = nullptr;
};

static int giql_hip_disjoin_plan_dev_impl(giql_hip_ctx* ctx, const giql_side* t, const giql_side* r, int32_t n_chrom,
                                          int64_t* n_out, void* stream) {
  if (!ctx || !n_out) return set_err(GIQL_ERR_INVALID, "ctx/n_out is NULL");
  GIQL_TRY(check_side(t, "target"));
  if (r) GIQL_TRY(check_side(r, "reference"));
  if (n_chrom < 0) return set_err(GIQL_ERR_INVALID, "n_chrom < 0");
  const bool self = r == nullptr;  // the reference defaults to the target: every piece is covered by its parent
  const giql_side* ref = self ? t : r;
  if ((u64)ref->n * 2 > OS_MAX_ROWS) return set_err(GIQL_ERR_INVALID, "DISJOIN reference larger than 2^29 rows");
  GIQL_TRY(begin_call(ctx, t->n, ref->n));
  hipStream_t st = (hipStream_t)stream;
  *n_out = 0;
  if (t->n == 0) return GIQL_OK;
  if (n_chrom == 0) return set_err(GIQL_ERR_CHROM, "rows but n_chrom = 0");
  const size_t nt = (size_t)t->n, nr = (size_t)ref->n, nev = 2 * nr;
  DisjoinBufs W;
  auto carve = [&](char* base) {
    Carver c{base};
    event_sizes(c, n_chrom, nev, W);
    W.bsums = c.take<u64>(cdiv((u64)(nev + 1 > nt ? nev + 1 : nt), SCAN_TILE) + 1);
    W.n_bp = c.take<u64>(1);
    W.scratch_total = c.take<u64>(1);
    W.total = c.take<u64>(1);
    W.bp = c.take<u32>(nev + 1);
    if (!self) {
      W.cov = c.take<u32>(nev + 1);
      W.ncov = c.take<u32>(nev + 1);
      W.cbp = c.take<u32>(nev + 1);
    }
    W.cnt = c.take<u32>(nt);
    W.lo_first = c.take<u32>(nt);
    W.off = c.take<u64>(nt + 1);
    return c.off;
  };
  GIQL_TRY(claim_arena(ctx, st, carve));
  GIQL_TRY(run_events(ctx, st, *t, r, n_chrom, W, "disjoin"));
  if (!self) HIP_TRY(hipMemsetAsync(W.cov, 0, (nev + 1) * sizeof(u32), st));
  if (nev > 0) {
    Phase ph(ctx, st, GIQL_PH_AUX, 1);
    ctx->stats.phase_bytes[GIQL_PH_AUX] += (int64_t)20 * nev + (int64_t)(self ? 4 : 8) * nev;  // (at most: every key distinct)
    hipLaunchKernelGGL(k_dj_compact, dim3(cdiv(nev, 256)), dim3(256), 0, st, W.sb.key[0], W.last, W.last_excl,
                       W.is_start, W.start_excl, (u32)nev, W.bp, W.cov);
    GIQL_TRY(post_launch("disjoin breakpoints"));
  }
  if (!self) {
    GIQL_TRY(run_scan<u32>(ctx, st, GIQL_PH_SCAN, W.cov, (u64)nev + 1, W.ncov, W.bsums, W.scratch_total));
    if (nev > 0) {
      Phase ph(ctx, st, GIQL_PH_AUX, 1);
      ctx->stats.phase_bytes[GIQL_PH_AUX] += (int64_t)12 * nev;
      hipLaunchKernelGGL(k_dj_covered, dim3(cdiv(nev, 256)), dim3(256), 0, st, W.cov, W.ncov, (u32)nev, W.cbp);
      GIQL_TRY(post_launch("disjoin covered breakpoints"));
    }
  }
  {
    Phase ph(ctx, st, GIQL_PH_COUNT, 1);
    ctx->stats.phase_bytes[GIQL_PH_COUNT] += (int64_t)20 * nt;  // three columns read, count + first breakpoint written
    hipLaunchKernelGGL(k_dj_count, dim3(cdiv(nt, 256)), dim3(256), 0, st, view_of(*t), n_chrom, W.lb.chrom_base, W.bp,
                       W.n_bp, self ? (const u32*)nullptr : W.cov, self ? (const u32*)nullptr : W.ncov, W.cnt,
                       W.lo_first, ctx->d_meta);
    GIQL_TRY(post_launch("disjoin count"));
  }
  GIQL_TRY(run_scan<u64>(ctx, st, GIQL_PH_SCAN, W.cnt, (u64)nt, W.off, W.bsums, W.total, &ctx->d_meta->n_out));
  GIQL_TRY(finish_events(ctx, st, DJ_BAD_TARGET | DJ_BAD_REFERENCE));
  collect_spans(ctx);
  DisjoinPlan& P = ctx->dj;
  P.target = *t;
  P.total = ctx->h_meta->n_out;
  P.chrom_base = W.lb.chrom_base;
  P.off = W.off;
  P.lo_first = W.lo_first;
  P.bp = W.bp;
  P.n_bp = W.n_bp;
  P.ncov = self ? nullptr : W.ncov;
  P.cbp = self ? nullptr : W.cbp;
  ctx->kept = Plan::DISJOIN;
  *n_out = (int64_t)P.total;
  ctx->stats.n_out = (int64_t)P.total;
  ctx->stats.span = (int64_t)ctx->h_meta->total_span;
  return GIQL_OK;
}

int giql_hip_disjoin_plan_dev(giql_hip_ctx* ctx, const giql_side* target, const giql_side* reference, int32_t n_chrom,
                              int64_t* n_out, void* stream) {
  return with_order_fallback(ctx, [&] { return giql_hip_disjoin_plan_dev_impl(ctx, target, reference, n_chrom, n_out, stream); });
}

int giql_hip_disjoin_fill_dev(giql_hip_ctx* ctx, int32_t* parent_out, int32_t* start_out, int32_t* end_out,
                              int64_t capacity, void* stream) {
  if (!ctx) return set_err(GIQL_ERR_INVALID, "ctx is NULL");
  const DisjoinPlan& P = ctx->dj;
  if (ctx->kept != Plan::DISJOIN) return set_err(GIQL_ERR_STATE, "disjoin_fill without a successful disjoin_plan");
  if (P.total == 0) return GIQL_OK;
  if (!parent_out || !start_out || !end_out) return set_err(GIQL_ERR_INVALID, "output buffer is NULL");
  if (capacity < 0 || (u64)capacity < P.total)
    return set_err(GIQL_ERR_CAPACITY, "capacity %lld < %llu rows", (long long)capacity, (unsigned long long)P.total);
  const u64 n_tiles = (P.total + DJ_FILL_TILE - 1) / DJ_FILL_TILE;
  if (n_tiles > 0x7FFFFFFFull) return set_err(GIQL_ERR_CAPACITY, "%llu output rows: more than one fill launch holds", (unsigned long long)P.total);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const int vec = (((uintptr_t)parent_out | (uintptr_t)start_out | (uintptr_t)end_out) & 15u) == 0 ? 1 : 0;
  {
    Phase ph(ctx, st, GIQL_PH_FILL, 1);
    ctx->stats.phase_bytes[GIQL_PH_FILL] += (int64_t)12 * (int64_t)P.total;  // three int32 outputs per row
    hipLaunchKernelGGL(k_dj_fill, dim3((u32)n_tiles), dim3(DJ_FILL_NT), 0, st, view_of(P.target), P.chrom_base, P.off,
                       P.total, P.lo_first, P.bp, P.n_bp, P.ncov, P.cbp, vec, parent_out, start_out, end_out);
    GIQL_TRY(post_launch("disjoin fill"));
  }
  return GIQL_OK;
}

// ------------------------------------------------------- coverage segments
// include/giql_hip_coverage.h.  DISJOIN's front in self mode (run_events: spans -> 2n event keys -> ONE (key, id) sort
// -> the two flag scans), then coverage_kernels.hip.h: breakpoints with their whole depth -> keep flags -> scan -> one row per kept
// breakpoint.  No per-row count, no offsets, no output-major fill: the output has at most 2n - 1 rows.
static int giql_hip_coverage_dev_impl(giql_hip_ctx* ctx, const giql_side* s, int32_t n_chrom, uint32_t flags,
                                      int32_t* chrom_out, int32_t* start_out, int32_t* end_out, int64_t* depth_out,
                                      int64_t capacity, int64_t* n_out, void* stream) {
  if (!ctx || !n_out) return set_err(GIQL_ERR_INVALID, "ctx/n_out is NULL");
  GIQL_TRY(check_side(s, "side"));
  if (n_chrom < 0) return set_err(GIQL_ERR_INVALID, "n_chrom < 0");
  if (flags & ~GIQL_COV_RUNS) return set_err(GIQL_ERR_INVALID, "coverage: unknown flags 0x%x", flags);
  if ((u64)s->n * 2 > OS_MAX_ROWS) return set_err(GIQL_ERR_INVALID, "coverage of a table larger than 2^29 rows");
  GIQL_TRY(begin_call(ctx, s->n));
  hipStream_t st = (hipStream_t)stream;
  *n_out = 0;
  if (s->n == 0) return GIQL_OK;
  if (n_chrom == 0) return set_err(GIQL_ERR_CHROM, "rows but n_chrom = 0");
  const bool runs = (flags & GIQL_COV_RUNS) != 0;
  const size_t n = (size_t)s->n, nev = 2 * n;
  EventBufs E;
  u32 *keep = nullptr, *slot = nullptr;
  u64* total = nullptr;
  auto carve = [&](char* base) {
    Carver c{base};
    event_sizes(c, n_chrom, nev, E);
    keep = c.take<u32>(nev);
    slot = c.take<u32>(nev + 1);
    E.bsums = c.take<u64>(cdiv((u64)nev + 1, SCAN_TILE) + 1);
    E.n_bp = c.take<u64>(1);
    E.scratch_total = c.take<u64>(1);
    total = c.take<u64>(1);
    return c.off;
  };
  GIQL_TRY(claim_arena(ctx, st, carve));
  GIQL_TRY(run_events(ctx, st, *s, nullptr, n_chrom, E, "coverage"));
  // The sort is done: its second buffers are free, and hold the breakpoints and their depths (at most nev of each).
  u32 *bp = E.sb.key[1], *depth = E.sb.rid[1];
  HIP_TRY(hipMemsetAsync(keep, 0, nev * sizeof(u32), st));  // (the scan runs over nev flags, the breakpoints are fewer)
  {
    Phase ph(ctx, st, GIQL_PH_AUX, runs ? 2 : 1);
    ctx->stats.phase_bytes[GIQL_PH_AUX] += (int64_t)(runs ? 40 : 32) * nev;  // (at most: every key distinct)
    hipLaunchKernelGGL(k_cov_depth, dim3(cdiv(nev, 256)), dim3(256), 0, st, E.sb.key[0], E.last, E.last_excl, E.is_start,
                       E.start_excl, (u32)nev, bp, depth, runs ? (u32*)nullptr : keep);
    if (runs) hipLaunchKernelGGL(k_cov_run_heads, dim3(cdiv(nev, 256)), dim3(256), 0, st, depth, E.n_bp, keep);
    GIQL_TRY(post_launch("coverage breakpoints"));
  }
  GIQL_TRY(run_scan<u32>(ctx, st, GIQL_PH_SCAN, keep, (u64)nev, slot, E.bsums, total, &ctx->d_meta->n_out));
  GIQL_TRY(finish_events(ctx, st, DJ_BAD_TARGET));  // (the text is DISJOIN's: coverage is its GROUP BY)
  const u64 h_total = ctx->h_meta->n_out;
  *n_out = (int64_t)h_total;
  if (capacity < 0 || (u64)capacity < h_total) {
    collect_spans(ctx);
    return set_err(GIQL_ERR_CAPACITY, "%llu coverage rows, capacity %lld", (unsigned long long)h_total, (long long)capacity);
  }
  if (h_total) {
    if (!chrom_out || !start_out || !end_out) return set_err(GIQL_ERR_INVALID, "output buffer is NULL");
    Phase ph(ctx, st, GIQL_PH_FILL, 1);
    ctx->stats.phase_bytes[GIQL_PH_FILL] += (int64_t)16 * nev + (int64_t)(depth_out ? 20 : 12) * (int64_t)h_total;
    hipLaunchKernelGGL(k_cov_fill, dim3(cdiv(nev, 256)), dim3(256), 0, st, bp, depth, keep, slot, E.n_bp, E.lb.chrom_first,
                       E.lb.chrom_base, n_chrom, (int)s->start_off, (int)s->end_off, runs ? 1 : 0, (u32)h_total, chrom_out,
                       start_out, end_out, (i64*)depth_out);
    GIQL_TRY(post_launch("coverage rows"));
  }
  HIP_TRY(hipStreamSynchronize(st));
  collect_spans(ctx);
  ctx->stats.n_out = (int64_t)h_total;
  ctx->stats.span = (int64_t)ctx->h_meta->total_span;
  return GIQL_OK;
}

int giql_hip_coverage_dev(giql_hip_ctx* ctx, const giql_side* side, int32_t n_chrom, uint32_t flags, int32_t* chrom_out,
                          int32_t* start_out, int32_t* end_out, int64_t* depth_out, int64_t capacity, int64_t* n_out,
                          void* stream) {
  return with_order_fallback(ctx, [&] {
    return giql_hip_coverage_dev_impl(ctx, side, n_chrom, flags, chrom_out, start_out, end_out, depth_out, capacity, n_out, stream);
  });
}

// ------------------------------------------------------- CONTAINS / WITHIN
// contain(outer, inner): the pairs with the inner row inside the outer one (src/giql/expanders/intersects.py:155-166;
// contain_kernels.hip.h).  Count-then-fill like the INNER pair.  Stages: spans of both sides on one axis -> ONE read of
// the length ranges (the form) -> linearize + (key, end, rid) sort of both sides -> candidate range per sorted outer
// row -> u64 offsets; then either the INNER join's k_partition + k_fill tail (uniform inner side: the range is exact)
// or the candidate-tile count -> u64 scan of the tile totals, with the candidate-tile fill in contain_fill.
struct ContainBufs {
  LinBufs lb;
  OsScratch os_o, os_i;
  u32 *wlo = nullptr, *cand = nullptr, *irr_cnt = nullptr, *extra = nullptr;
  u64* bsums = nullptr;
};

// The candidate stage shared by the CONTAINS plan and the per-row containment counts: workspace, spans, the form,
// both sorts, the candidate range {P.lo, W.cand} of every sorted outer row and their u64 offsets P.coff, with the
// total read back (uniform form: the pairs, DevMeta::n_out; general form: the candidates, DevMeta::n_out_c1).
// extra_words: u32 words carved for the caller behind the stage's own buffers (W.extra); force_general: take the
// candidate-tile form whatever the inner side's lengths are.
static int contain_candidates(giql_hip_ctx* ctx, hipStream_t st, const giql_side* o, const giql_side* in,
                              int32_t n_chrom, ContainPlan& P, ContainBufs& W, size_t extra_words,
                              bool force_general) {
  const size_t no = (size_t)o->n, ni = (size_t)in->n, nq = no + ni;
  if (no > OS_MAX_ROWS || ni > OS_MAX_ROWS) return set_err(GIQL_ERR_INVALID, "side larger than 2^30 rows");
  constexpr u32 TQ = RC_NT * RC_ITEMS_C2;
  const u32 nt = cdiv(no, TQ);
  auto carve = [&](char* base) {
    Carver c{base};
    common_sizes(c, n_chrom, W.lb);
    sort_sizes(c, no, P.so, true);
    sort_sizes(c, ni, P.si, true);
    os_scratch_sizes(c, no, W.os_o);
    os_scratch_sizes(c, ni, W.os_i);
    P.irr_o_list = c.take<u32>(no);
    P.irr_i_list = c.take<u32>(ni);
    W.wlo = c.take<u32>((size_t)nt + 2);
    P.lo = c.take<u32>(no);
    W.cand = c.take<u32>(no);
    P.coff = c.take<u64>(no + 1);
    W.irr_cnt = c.take<u32>(nq);
    P.irr_off = c.take<u64>(nq + 1);
    W.bsums = c.take<u64>(cdiv(nq, SCAN_TILE) + 2);
    W.extra = c.take<u32>(extra_words);
    return c.off;
  };
  GIQL_TRY(claim_arena(ctx, st, carve));
  GIQL_TRY(run_spans(ctx, st, *o, *in, n_chrom, W.lb));
  // the ONE read that decides the form (and reports a bad chromosome id or an axis past 32 bits before anything is
  // sorted).  Uniform inner side: min == max canonical length > 0 over ALL its rows -- a single irregular row makes
  // the minimum 0 (decide_form).
  GIQL_TRY(read_meta(ctx, st));
  ctx->guess.last_span = ctx->h_meta->total_span;  // known before anything is sorted: the sort form follows the real density
  const i64 uni_len = (ctx->sw.no_uniform || force_general) ? 0 : uniform_len_b(*ctx->h_meta);
  P.form = uni_len > 0 ? 1 : 0;
  GIQL_TRY(run_linearize(ctx, st, *o, n_chrom, W.lb, Side::A, LinTarget::keys_ends(P.so.key[0], P.so.end[0], P.irr_o_list),
                         LinOptions().counting_starts(W.os_o.starts())));
  GIQL_TRY(run_sort_onesweep(ctx, st, P.so, sort_by_start(W.os_o, no)));
  if (P.form == 1) {
    // every inner row is regular and uni_len long: keys and row ids only, its `end` column is not read again
    P.si.end[0] = P.si.end[1] = nullptr;
    GIQL_TRY(run_linearize(ctx, st, *in, n_chrom, W.lb, Side::B, LinTarget::keys_only(P.si.key[0], P.irr_i_list),
                           LinOptions().counting_starts(W.os_i.starts()).without_end_column()));
  } else {
    GIQL_TRY(run_linearize(ctx, st, *in, n_chrom, W.lb, Side::B, LinTarget::keys_ends(P.si.key[0], P.si.end[0], P.irr_i_list),
                           LinOptions().counting_starts(W.os_i.starts())));
  }
  GIQL_TRY(run_sort_onesweep(ctx, st, P.si, sort_by_start(W.os_i, ni)));
  const u32* irr_o = &ctx->d_meta->irr_a;
  const u32* irr_i = &ctx->d_meta->irr_b;
  {
    // Candidates of a sorted outer row c: the inner keys in [c.key, c.endkey) -- the class-1 range, lo_off = 0 (uniform
    // form: in [c.key, c.endkey - L + 1), which is exact).  The range cannot leak into the next chromosome:
    // k_chrom_offsets gives each chromosome max - min + 1 positions over both sides, so an end key never reaches the
    // next chromosome's base and every inner key below c.endkey lies on c's chromosome.
    Phase ph(ctx, st, GIQL_PH_COUNT, 2);
    ctx->stats.phase_bytes[GIQL_PH_COUNT] += (int64_t)16 * no + (int64_t)4 * ni;  // keys + ends read, lo + cand written; the inner keys
    hipLaunchKernelGGL(k_count_partition, dim3(cdiv((u64)nt + 1, 256)), dim3(256), 0, st, P.so.key[0], (u32)no, irr_o,
                       P.si.key[0], (u32)ni, irr_i, (i64)0, TQ, nt, W.wlo);
    if (P.form == 1)
      hipLaunchKernelGGL((k_contain_range_count<RC_ITEMS_C2, RC_LDS_CAP>), dim3(nt), dim3(RC_NT), 0, st, P.so.key[0],
                         P.so.end[0], (u32)no, irr_o, P.si.key[0], (u32)ni, irr_i, (i64)1 - uni_len, W.wlo, P.lo, W.cand);
    else
      hipLaunchKernelGGL((k_range_count<RC_ITEMS_C2, RC_LDS_CAP>), dim3(nt), dim3(RC_NT), 0, st, P.so.key[0],
                         P.so.end[0], (u32)no, irr_o, P.si.key[0], (u32)ni, irr_i, (i64)0, W.wlo, P.lo, W.cand);
    GIQL_TRY(post_launch("contain range count"));
  }
  // uniform form: the counts are the pairs (n_out); general form: the candidates (n_out_c1)
  GIQL_TRY(run_scan<u64>(ctx, st, GIQL_PH_SCAN, W.cand, (u64)no, P.coff, W.bsums, P.coff + no,
                         P.form == 1 ? &ctx->d_meta->n_out : &ctx->d_meta->n_out_c1));
  GIQL_TRY(read_meta(ctx, st));
  return GIQL_OK;
}

static int giql_hip_contain_plan_dev_impl(giql_hip_ctx* ctx, const giql_side* o, const giql_side* in, int32_t n_chrom,
                                          void* stream, int64_t* n_pairs) {
  if (!ctx || !n_pairs) return set_err(GIQL_ERR_INVALID, "ctx/n_pairs is NULL");
  GIQL_TRY(check_side(o, "outer"));
  GIQL_TRY(check_side(in, "inner"));
  if (n_chrom < 0) return set_err(GIQL_ERR_INVALID, "n_chrom < 0");
  GIQL_TRY(begin_call(ctx, o->n, in->n));
  hipStream_t st = (hipStream_t)stream;
  ContainPlan& P = ctx->ct;
  P = ContainPlan{};
  P.outer = *o;
  P.inner = *in;
  P.n_o = (u32)o->n;
  P.n_i = (u32)in->n;
  *n_pairs = 0;
  if (o->n == 0 || in->n == 0) {  // nothing to launch
    ctx->kept = Plan::CONTAINS;
    return GIQL_OK;
  }
  if (n_chrom == 0) return set_err(GIQL_ERR_CHROM, "rows but n_chrom = 0");
  const size_t no = (size_t)o->n, ni = (size_t)in->n, nq = no + ni;
  ContainBufs W;
  GIQL_TRY(contain_candidates(ctx, st, o, in, n_chrom, P, W, 0, false));
  if (P.form == 1) {
    P.n_reg = ctx->h_meta->n_out;
  } else {
    P.n_cand = ctx->h_meta->n_out_c1;
    const u64 n_tiles = (P.n_cand + CT_TILE - 1) / CT_TILE;
    if (n_tiles > 0x7FFFFFFFull)
      return set_err(GIQL_ERR_CAPACITY, "%llu candidate pairs: more than one launch holds", (unsigned long long)P.n_cand);
    P.n_tiles = (u32)n_tiles;
    if (n_tiles > 0) {
      u32* tile_cnt = nullptr;
      u64* bsums_t = nullptr;
      auto carve_t = [&](char* base) {
        Carver c{base};
        P.ct_part = c.take<u32>((size_t)n_tiles + 2);
        tile_cnt = c.take<u32>((size_t)n_tiles);
        P.tile_off = c.take<u64>((size_t)n_tiles + 1);
        bsums_t = c.take<u64>(cdiv(n_tiles, SCAN_TILE) + 2);
        return c.off;
      };
      const size_t need = carve_t(nullptr);
      GIQL_TRY(ctx->ct_buf.grow(need, need + need / 4, st, "the candidate tiles"));
      carve_t(ctx->ct_buf);
      {
        Phase ph(ctx, st, GIQL_PH_PARTITION);
        hipLaunchKernelGGL(k_partition, dim3(cdiv(n_tiles + 1, 256)), dim3(256), 0, st, P.coff, (u32)no, (u64)0, CT_TILE,
                           P.n_tiles, P.ct_part);
      }
      {
        Phase ph(ctx, st, GIQL_PH_COUNT);
        // every candidate's inner end read once; the tiles' row records {offset, lo, end}; one total per tile
        ctx->stats.phase_bytes[GIQL_PH_COUNT] += (int64_t)4 * (int64_t)P.n_cand + (int64_t)16 * no + (int64_t)4 * (int64_t)n_tiles;
        hipLaunchKernelGGL(k_ct_count, dim3(P.n_tiles), dim3(CT_NT), 0, st, P.coff, P.lo, P.so.end[0], (u32)no,
                           P.si.end[0], P.ct_part, P.n_cand, tile_cnt);
        GIQL_TRY(post_launch("contain tile count"));
      }
      GIQL_TRY(run_scan<u64>(ctx, st, GIQL_PH_SCAN, tile_cnt, n_tiles, P.tile_off, bsums_t, P.tile_off + n_tiles,
                             &ctx->d_meta->n_out));
      GIQL_TRY(read_meta(ctx, st));
      P.n_reg = ctx->h_meta->n_out;
    }
  }
  ctx->stats.n_irregular_a = ctx->h_meta->irr_a;
  ctx->stats.n_irregular_b = ctx->h_meta->irr_b;
  if (ctx->h_meta->irr_a + ctx->h_meta->irr_b > 0) {
    {
      Phase ph(ctx, st, GIQL_PH_IRREGULAR);
      ctx->stats.phase_bytes[GIQL_PH_IRREGULAR] += (int64_t)16 * (int64_t)nq;  // three columns read, one count written (+ the listed rows)
      hipLaunchKernelGGL(k_contain_irr_count, dim3(cdiv(nq, 256)), dim3(256), 0, st, view_of(*o), view_of(*in),
                         P.irr_o_list, P.irr_i_list, ctx->d_meta, W.irr_cnt);
      GIQL_TRY(post_launch("contain irregular count"));
    }
    GIQL_TRY(run_scan<u64>(ctx, st, GIQL_PH_IRREGULAR, W.irr_cnt, (u64)nq, P.irr_off, W.bsums, P.irr_off + nq,
                           &ctx->d_meta->n_out_irr));
    GIQL_TRY(read_meta(ctx, st));
    P.n_irr = ctx->h_meta->n_out_irr;
  }
  collect_spans(ctx);
  ctx->stats.reserved = P.form;  // join_form: 0 general (candidate tiles), 1 uniform inner side
  ctx->stats.n_out = (int64_t)(P.n_reg + P.n_irr);
  ctx->stats.span = (int64_t)ctx->h_meta->total_span;
  *n_pairs = (int64_t)(P.n_reg + P.n_irr);
  ctx->kept = Plan::CONTAINS;
  return GIQL_OK;
}

int giql_hip_contain_plan_dev(giql_hip_ctx* ctx, const giql_side* outer, const giql_side* inner, int32_t n_chrom,
                              void* stream, int64_t* n_pairs) {
  return with_order_fallback(ctx, [&] { return giql_hip_contain_plan_dev_impl(ctx, outer, inner, n_chrom, stream, n_pairs); });
}

int giql_hip_contain_fill_dev(giql_hip_ctx* ctx, int32_t* row_outer, int32_t* row_inner, int64_t capacity,
                              void* stream) {
  if (!ctx) return set_err(GIQL_ERR_INVALID, "ctx is NULL");
  const ContainPlan& P = ctx->ct;
  if (ctx->kept != Plan::CONTAINS) return set_err(GIQL_ERR_STATE, "contain_fill without a successful contain_plan");
  const u64 total = P.n_reg + P.n_irr;
  if (total == 0) return GIQL_OK;
  if (!row_outer || !row_inner) return set_err(GIQL_ERR_INVALID, "row_outer/row_inner is NULL");
  if (capacity < 0 || (u64)capacity < total)
    return set_err(GIQL_ERR_CAPACITY, "capacity %lld < %llu pairs", (long long)capacity, (unsigned long long)total);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  if (P.n_reg > 0 && P.form == 1) {
    constexpr u32 T2 = FILL_NT * FILL_ITEMS_C2;
    const u64 nt64 = (P.n_reg + T2 - 1) / T2;
    if (nt64 > 0x7FFFFFF0ull)
      return set_err(GIQL_ERR_CAPACITY, "%llu pairs: more than one fill launch holds", (unsigned long long)P.n_reg);
    const u32 ntf = (u32)nt64;
    GIQL_TRY(grow_part(ctx, (size_t)ntf + 2, st));
    {
      Phase ph(ctx, st, GIQL_PH_PARTITION);
      hipLaunchKernelGGL(k_partition, dim3(cdiv((u64)ntf + 1, 256)), dim3(256), 0, st, P.coff, P.n_o, (u64)0, T2, ntf,
                         ctx->part);
    }
    Phase ph(ctx, st, GIQL_PH_FILL);
    ctx->stats.phase_bytes[GIQL_PH_FILL] += (int64_t)12 * (int64_t)P.n_reg + (int64_t)16 * P.n_o;  // rid gather + two outputs; the row records
    hipLaunchKernelGGL((k_fill<FILL_ITEMS_C2>), dim3(ntf), dim3(FILL_NT), 0, st, P.coff, P.lo, P.so.rid[0], P.n_o,
                       P.si.rid[0], ctx->part, (u64)0, P.n_reg, row_outer, row_inner);
    GIQL_TRY(post_launch("contain fill (uniform inner side)"));
  } else if (P.n_reg > 0) {
    Phase ph(ctx, st, GIQL_PH_FILL);
    // the count pass's reads again + the tile offsets, a rid gather and two outputs per pair
    ctx->stats.phase_bytes[GIQL_PH_FILL] += (int64_t)4 * (int64_t)P.n_cand + (int64_t)20 * P.n_o +
                                            (int64_t)8 * P.n_tiles + (int64_t)12 * (int64_t)P.n_reg;
    hipLaunchKernelGGL(k_ct_fill, dim3(P.n_tiles), dim3(CT_NT), 0, st, P.coff, P.lo, P.so.end[0], P.so.rid[0], P.n_o,
                       P.si.end[0], P.si.rid[0], P.ct_part, P.n_cand, P.tile_off, row_outer, row_inner);
    GIQL_TRY(post_launch("contain fill (candidate tiles)"));
  }
  if (P.n_irr > 0) {
    Phase ph(ctx, st, GIQL_PH_IRREGULAR);
    ctx->stats.phase_bytes[GIQL_PH_IRREGULAR] += (int64_t)8 * (int64_t)P.n_irr + (int64_t)20 * ((int64_t)P.n_o + P.n_i);
    hipLaunchKernelGGL(k_contain_irr_fill, dim3(cdiv((u64)P.n_o + P.n_i, 256)), dim3(256), 0, st, view_of(P.outer),
                       view_of(P.inner), P.irr_o_list, P.irr_i_list, ctx->d_meta, P.irr_off, row_outer + P.n_reg,
                       row_inner + P.n_reg);
    GIQL_TRY(post_launch("contain irregular fill"));
  }
  return GIQL_OK;
}

// ------------------------------------- SEMI / ANTI / COUNT over CONTAINS, WITHIN, DISTANCE
// The per-row forms of the three pair predicates that are not INTERSECTS (row_pred_kernels.hip.h).  Nothing is
// speculated: every call reads the span pass back once (chrom ids, the 32-bit axis, inverted rows under DISTANCE)
// before it sorts.
static int check_rowpred(int32_t pred, int64_t max_distance) {
  if (pred != GIQL_ROWPRED_CONTAINS && pred != GIQL_ROWPRED_WITHIN && pred != GIQL_ROWPRED_DISTANCE)
    return set_err(GIQL_ERR_INVALID, "pred %d is none of GIQL_ROWPRED_*", (int)pred);
  if (pred == GIQL_ROWPRED_DISTANCE && max_distance < -1) return set_err(GIQL_ERR_INVALID, "max_distance < -1");
  return GIQL_OK;
}

// The exit of a call whose right side can pair with no left row: nothing for SEMI, every row for ANTI.
static int every_row_for_anti(giql_hip_ctx* ctx, hipStream_t st, size_t na, int anti, int32_t* rows_out, int64_t* n_out,
                              const char* what) {
  if (anti) {
    hipLaunchKernelGGL(k_rp_iota, dim3(cdiv(na, 256)), dim3(256), 0, st, rows_out, (u32)na);
    GIQL_TRY(post_launch(what));
    *n_out = (int64_t)na;
  }
  ctx->stats.n_out = *n_out;
  return GIQL_OK;
}

static int giql_hip_semi_anti_pred_dev_impl(giql_hip_ctx* ctx, const giql_side* a, const giql_side* b, int32_t n_chrom,
                                            int32_t pred, int64_t max_distance, int anti, int32_t* rows_out,
                                            int64_t* n_out, void* stream) {
  if (!ctx || !n_out) return set_err(GIQL_ERR_INVALID, "ctx/n_out is NULL");
  GIQL_TRY(check_rowpred(pred, max_distance));
  GIQL_TRY(begin_pair_call(ctx, a, b, n_chrom));
  hipStream_t st = (hipStream_t)stream;
  *n_out = 0;
  if (a->n == 0) return GIQL_OK;
  if (!rows_out) return set_err(GIQL_ERR_INVALID, "rows_out is NULL");
  const size_t na = (size_t)a->n, nb = (size_t)b->n;
  GIQL_TRY(check_rows_fit(na, nb));
  if (nb > 0 && n_chrom == 0) return set_err(GIQL_ERR_CHROM, "rows but n_chrom = 0");
  const bool dist = pred == GIQL_ROWPRED_DISTANCE;
  const int nch = n_chrom;
  if (nb == 0) return every_row_for_anti(ctx, st, na, anti, rows_out, n_out, "anti (empty right side)");

  LinBufs lb;
  SortBufs sa, sbb;
  OsScratchPair osp;
  OsScratch &os_a = osp.a, &os = osp.b;
  u32 *flag = nullptr, *pmax = nullptr, *bmax = nullptr, *dummy_irr = nullptr;
  u64 *bsums = nullptr, *off = nullptr;
  auto carve = [&](char* base) {
    Carver c{base};
    common_sizes(c, nch, lb);
    sort_sizes(c, na, sa, true);
    sort_sizes_key_payload(c, nb, sbb);  // B: (sort key, the other key as payload)
    os_pair_sizes(c, na, nb, osp);
    bsums = c.take<u64>(cdiv(na, SCAN_TILE) + 2);
    flag = c.take<u32>(na);
    off = c.take<u64>(na + 1);
    pmax = c.take<u32>(nb);
    bmax = c.take<u32>(cdiv(nb, PM_TILE) + 1);
    dummy_irr = c.take<u32>(16);
    return c.off;
  };
  GIQL_TRY(claim_arena(ctx, st, carve));
  GIQL_TRY(run_spans(ctx, st, *a, *b, nch, lb, -1, nullptr, /*pad=*/dist ? 1 : 0));
  GIQL_TRY(read_meta(ctx, st));
  if (dist) GIQL_TRY(reject_inverted(ctx));
  note_span(ctx);
  if (dist && max_distance < 0)  // `< 0`: no pair, after the rows have been checked
    return every_row_for_anti(ctx, st, na, anti, rows_out, n_out, "anti (no pair possible)");
  // A: every row on its real key, sorted coarsely (its order only serves locality)
  if (dist) {
    GIQL_TRY(key_widened_side(ctx, st, *a, *b, nch, lb, clamp_widen(max_distance), sa, nullptr, os_a.hist, os_a.gbase));
  } else {
    GIQL_TRY(run_linearize(ctx, st, *a, nch, lb, Side::A, LinTarget::keys_ends(sa.key[0], sa.end[0], dummy_irr + 8),
                           LinOptions().keeping_irregular().counting_starts(os_a.starts())));
  }
  GIQL_TRY(run_sort_onesweep(ctx, st, sa, sort_by_start(os_a, na).skipping_digits(row_skip(sort_tuning(ctx), nb))));
  // B: every row on its real key.  WITHIN and DISTANCE sort it by start with the end keys as payload; CONTAINS sorts
  // it by END with the start keys as payload -- a SortBufs is only pointers, and the linearize pass counts the end
  // keys' digits on the way (os.hist_e / os.gbase_e, as the COUNT path's second sort does).
  if (pred == GIQL_ROWPRED_CONTAINS) {
    // (the start keys land in the PAYLOAD array, the end keys in the key array)
    GIQL_TRY(run_linearize(ctx, st, *b, nch, lb, Side::B, LinTarget::keys_ends(sbb.end[0], sbb.key[0], dummy_irr),
                           LinOptions().keeping_irregular().counting_starts(os.starts()).counting_ends(os.ends())));
    GIQL_TRY(run_sort_onesweep(ctx, st, sbb, sort_by_end(os, nb)));
  } else {
    GIQL_TRY(run_linearize(ctx, st, *b, nch, lb, Side::B, LinTarget::keys_ends(sbb.key[0], sbb.end[0], dummy_irr),
                           LinOptions().keeping_irregular().counting_starts(os.starts())));
    GIQL_TRY(run_sort_onesweep(ctx, st, sbb, sort_by_start(os, nb)));
  }
  GIQL_TRY(run_pmax(ctx, st, sbb.end[0], (u32)nb, pmax, bmax));
  {
    Phase ph(ctx, st, GIQL_PH_COUNT);
    if (dist)
      hipLaunchKernelGGL(k_semi_flags, dim3(cdiv(na, 256)), dim3(256), 0, st, sa.key[0], sa.end[0], sa.rid[0], (u32)na,
                         ctx->d_meta, sbb.key[0], pmax, (u32)nb, anti, flag);
    else
      hipLaunchKernelGGL(k_rp_semi_flags, dim3(cdiv(na, 256)), dim3(256), 0, st, sa.key[0], sa.end[0], sa.rid[0],
                         (u32)na, ctx->d_meta, sbb.key[0], pmax, (u32)nb, pred == GIQL_ROWPRED_WITHIN ? 1 : 0, anti,
                         flag);
    GIQL_TRY(post_launch("row predicate flags"));
  }
  GIQL_TRY(finish_semi(ctx, st, flag, na, bsums, off + na, rows_out));
  collect_spans(ctx);
  ctx->stats.reserved = 0;  // form: general, the only one
  *n_out = (int64_t)ctx->h_meta->n_out;
  ctx->stats.n_out = *n_out;
  return GIQL_OK;
}

int giql_hip_semi_anti_pred_dev(giql_hip_ctx* ctx, const giql_side* a, const giql_side* b, int32_t n_chrom,
                                int32_t pred, int64_t max_distance, int anti, int32_t* rows_out, int64_t* n_out,
                                void* stream) {
  return with_order_fallback(ctx, [&] {
    return giql_hip_semi_anti_pred_dev_impl(ctx, a, b, n_chrom, pred, max_distance, anti, rows_out, n_out, stream);
  });
}

// COUNT over DISTANCE: the rank difference of giql_hip_count_dev over the widened A (general form only).
static int count_window(giql_hip_ctx* ctx, hipStream_t st, const giql_side* a, const giql_side* b, int32_t n_chrom,
                        int64_t max_distance, int64_t* counts_out) {
  const size_t na = (size_t)a->n, nb = (size_t)b->n;
  LinBufs lb;
  SortBufs sa, sstart, send;
  OsScratchPair osp;
  OsScratch &os_a = osp.a, &os = osp.b;
  u32 *irr_a_list = nullptr, *irr_b_list = nullptr;
  auto carve = [&](char* base) {
    Carver c{base};
    common_sizes(c, n_chrom, lb);
    sort_sizes(c, na, sa, true);
    sort_sizes_starts_ends(c, nb, sstart, send);
    os_pair_sizes(c, na, nb, osp);
    irr_a_list = c.take<u32>(na);
    irr_b_list = c.take<u32>(nb);
    return c.off;
  };
  GIQL_TRY(claim_arena(ctx, st, carve));
  GIQL_TRY(run_spans(ctx, st, *a, *b, n_chrom, lb, -1, nullptr, /*pad=*/1));
  GIQL_TRY(read_meta(ctx, st));
  GIQL_TRY(reject_inverted(ctx));
  note_span(ctx);
  if (max_distance < 0) {  // `< 0`: no pair, after the rows have been checked
    HIP_TRY(hipMemsetAsync(counts_out, 0, na * sizeof(int64_t), st));
    ctx->stats.n_out = a->n;
    return GIQL_OK;
  }
  const i64 widen = clamp_widen(max_distance);
  GIQL_TRY(key_widened_side(ctx, st, *a, *b, n_chrom, lb, widen, sa, irr_a_list, os_a.hist, os_a.gbase));
  // locality only: the kernel tells listed rows by their key
  GIQL_TRY(run_sort_onesweep(ctx, st, sa, sort_by_start(os_a, na).skipping_digits(row_skip(sort_tuning(ctx), nb))));
  GIQL_TRY(run_linearize(ctx, st, *b, n_chrom, lb, Side::B, LinTarget::keys_ends(sstart.key[0], send.key[0], irr_b_list),
                         LinOptions().counting_starts(os.starts()).counting_ends(os.ends())));
  GIQL_TRY(run_sort_onesweep(ctx, st, sstart, sort_by_start(os, nb)));
  GIQL_TRY(run_sort_onesweep(ctx, st, send, sort_by_end(os, nb)));
  {
    Phase ph(ctx, st, GIQL_PH_COUNT);
    hipLaunchKernelGGL(k_rp_count_window_rows, dim3(cdiv(na, 256)), dim3(256), 0, st, sa.key[0], sa.end[0], sa.rid[0],
                       (u32)na, view_of(*a), view_of(*b), sstart.key[0], send.key[0], (u32)nb, irr_b_list, ctx->d_meta,
                       widen, counts_out);
    GIQL_TRY(post_launch("count rows (distance)"));
  }
  GIQL_TRY(read_meta(ctx, st));
  ctx->stats.n_irregular_a = ctx->h_meta->irr_a;
  ctx->stats.n_irregular_b = ctx->h_meta->irr_b;
  if (ctx->h_meta->irr_a > 0) {
    Phase ph(ctx, st, GIQL_PH_IRREGULAR);
    hipLaunchKernelGGL(k_rp_count_irregular, dim3(ctx->h_meta->irr_a), dim3(256), 0, st, view_of(*a), view_of(*b),
                       irr_a_list, (int)GIQL_ROWPRED_DISTANCE, widen, counts_out);
    GIQL_TRY(post_launch("count irregular (distance)"));
    HIP_TRY(hipStreamSynchronize(st));
  }
  collect_spans(ctx);
  ctx->stats.reserved = 0;
  ctx->stats.n_out = a->n;
  return GIQL_OK;
}

// COUNT over CONTAINS / WITHIN: the CONTAINS plan's candidate stage, then the per-row tile walk (k_ct_rows) or, with a
// uniform inner side under CONTAINS, the exact range counts scattered by row id.  a CONTAINS b: a is the outer side;
// a WITHIN b: a is the inner side, and the general form is taken whatever a's lengths are.
static int count_contain(giql_hip_ctx* ctx, hipStream_t st, const giql_side* a, const giql_side* b, int32_t n_chrom,
                         int32_t pred, int64_t* counts_out) {
  const bool per_inner = pred == GIQL_ROWPRED_WITHIN;
  const giql_side* o = per_inner ? b : a;
  const giql_side* in = per_inner ? a : b;
  const size_t no = (size_t)o->n, ni = (size_t)in->n, na = (size_t)a->n;
  ContainPlan P;  // a call's own: the context holds no plan afterwards
  ContainBufs W;
  P.n_o = (u32)no;
  P.n_i = (u32)ni;
  GIQL_TRY(contain_candidates(ctx, st, o, in, n_chrom, P, W, per_inner ? ni : 0, per_inner));
  // (listed rows: the outer side was linearised as side 0, the inner one as side 1)
  const u32 irr_o = ctx->h_meta->irr_a, irr_i = ctx->h_meta->irr_b;
  ctx->stats.n_irregular_a = per_inner ? irr_i : irr_o;
  ctx->stats.n_irregular_b = per_inner ? irr_o : irr_i;
  ctx->stats.span = (int64_t)ctx->h_meta->total_span;
  if (P.form == 1) {
    Phase ph(ctx, st, GIQL_PH_FILL);
    hipLaunchKernelGGL(k_rp_scatter_counts, dim3(cdiv(no, 256)), dim3(256), 0, st, W.cand, P.so.rid[0], (u32)no,
                       counts_out);
    GIQL_TRY(post_launch("count scatter (uniform inner side)"));
  } else {
    P.n_cand = ctx->h_meta->n_out_c1;
    const u64 n_tiles = (P.n_cand + CT_TILE - 1) / CT_TILE;
    if (n_tiles > 0x7FFFFFFFull)
      return set_err(GIQL_ERR_CAPACITY, "%llu candidate pairs: more than one launch holds", (unsigned long long)P.n_cand);
    if (per_inner)
      HIP_TRY(hipMemsetAsync(W.extra, 0, ni * sizeof(u32), st));
    else
      HIP_TRY(hipMemsetAsync(counts_out, 0, na * sizeof(int64_t), st));
    if (n_tiles > 0) {
      const size_t need = ((size_t)n_tiles + 2) * sizeof(u32);
      GIQL_TRY(ctx->ct_buf.grow(need, need + need / 4, st, "the candidate tiles"));
      P.ct_part = reinterpret_cast<u32*>((char*)ctx->ct_buf);
      {
        Phase ph(ctx, st, GIQL_PH_PARTITION);
        hipLaunchKernelGGL(k_partition, dim3(cdiv(n_tiles + 1, 256)), dim3(256), 0, st, P.coff, (u32)no, (u64)0, CT_TILE,
                           (u32)n_tiles, P.ct_part);
      }
      Phase ph(ctx, st, GIQL_PH_COUNT);
      ctx->stats.phase_bytes[GIQL_PH_COUNT] += (int64_t)4 * (int64_t)P.n_cand + (int64_t)20 * no;
      if (per_inner)
        hipLaunchKernelGGL(k_ct_rows<true>, dim3((u32)n_tiles), dim3(CT_NT), 0, st, P.coff, P.lo, P.so.end[0],
                           P.so.rid[0], (u32)no, P.si.end[0], P.ct_part, P.n_cand, (unsigned long long*)nullptr, W.extra);
      else
        hipLaunchKernelGGL(k_ct_rows<false>, dim3((u32)n_tiles), dim3(CT_NT), 0, st, P.coff, P.lo, P.so.end[0],
                           P.so.rid[0], (u32)no, P.si.end[0], P.ct_part, P.n_cand,
                           reinterpret_cast<unsigned long long*>(counts_out), (u32*)nullptr);
      GIQL_TRY(post_launch("contain row counts"));
    }
    if (per_inner) {
      Phase ph(ctx, st, GIQL_PH_FILL);
      hipLaunchKernelGGL(k_rp_scatter_counts, dim3(cdiv(ni, 256)), dim3(256), 0, st, W.extra, P.si.rid[0], (u32)ni,
                         counts_out);
      GIQL_TRY(post_launch("count scatter (per inner row)"));
    }
  }
  // rows the sorted prefixes leave out, by the literal predicate: (listed a) x (every b), (regular a) x (listed b)
  const u32 irr_x = per_inner ? irr_i : irr_o, irr_y = per_inner ? irr_o : irr_i;
  const u32* list_x = per_inner ? P.irr_i_list : P.irr_o_list;
  const u32* list_y = per_inner ? P.irr_o_list : P.irr_i_list;
  if (irr_x + irr_y > 0) {
    Phase ph(ctx, st, GIQL_PH_IRREGULAR, 2);
    if (irr_y > 0)
      hipLaunchKernelGGL(k_rp_count_vs_irregular, dim3(cdiv(na, 256)), dim3(256), 0, st, view_of(*a), view_of(*b),
                         list_y, per_inner ? &ctx->d_meta->irr_a : &ctx->d_meta->irr_b, (int)pred, counts_out);
    if (irr_x > 0)
      hipLaunchKernelGGL(k_rp_count_irregular, dim3(irr_x), dim3(256), 0, st, view_of(*a), view_of(*b), list_x,
                         (int)pred, (i64)0, counts_out);
    GIQL_TRY(post_launch("count irregular (containment)"));
  }
  HIP_TRY(hipStreamSynchronize(st));
  collect_spans(ctx);
  ctx->stats.reserved = P.form;  // form: 0 general (candidate tiles), 1 uniform inner side
  ctx->stats.n_out = a->n;
  return GIQL_OK;
}

static int giql_hip_count_pred_dev_impl(giql_hip_ctx* ctx, const giql_side* a, const giql_side* b, int32_t n_chrom,
                                        int32_t pred, int64_t max_distance, int64_t* counts_out, void* stream) {
  if (!ctx) return set_err(GIQL_ERR_INVALID, "ctx is NULL");
  GIQL_TRY(check_rowpred(pred, max_distance));
  GIQL_TRY(begin_pair_call(ctx, a, b, n_chrom));
  hipStream_t st = (hipStream_t)stream;
  if (a->n == 0) return GIQL_OK;
  if (!counts_out) return set_err(GIQL_ERR_INVALID, "counts_out is NULL");
  const size_t na = (size_t)a->n, nb = (size_t)b->n;
  GIQL_TRY(check_rows_fit(na, nb));
  if (nb > 0 && n_chrom == 0) return set_err(GIQL_ERR_CHROM, "rows but n_chrom = 0");
  if (nb == 0) {
    HIP_TRY(hipMemsetAsync(counts_out, 0, na * sizeof(int64_t), st));
    ctx->stats.n_out = a->n;
    return GIQL_OK;
  }
  if (pred == GIQL_ROWPRED_DISTANCE) return count_window(ctx, st, a, b, n_chrom, max_distance, counts_out);
  return count_contain(ctx, st, a, b, n_chrom, pred, counts_out);
}

int giql_hip_count_pred_dev(giql_hip_ctx* ctx, const giql_side* a, const giql_side* b, int32_t n_chrom, int32_t pred,
                            int64_t max_distance, int64_t* counts_out, void* stream) {
  return with_order_fallback(ctx, [&] {
    return giql_hip_count_pred_dev_impl(ctx, a, b, n_chrom, pred, max_distance, counts_out, stream);
  });
}

// ------------------------------------------- distinct intervals + segment sums
// (the aggregate half of count_overlaps: GROUP BY the left interval, SUM of the per-row
// counts -- src/giql/expanders/intersects_duckdb.py:806-854)
static int giql_hip_group_rows_dev_impl(giql_hip_ctx* ctx, const giql_side* s, int32_t n_chrom,
                                        int32_t* group_of_row, int32_t* rep_row, int64_t* n_groups,
                                        void* stream) {
  if (!ctx || !n_groups) return set_err(GIQL_ERR_INVALID, "ctx/n_groups is NULL");
  GIQL_TRY(check_side(s, "s"));
  if (n_chrom < 0) return set_err(GIQL_ERR_INVALID, "n_chrom < 0");
  GIQL_TRY(check_rows_fit((size_t)s->n, 0));
  GIQL_TRY(begin_call(ctx, s->n));
  hipStream_t st = (hipStream_t)stream;
  *n_groups = 0;
  if (s->n == 0) return GIQL_OK;
  if (!group_of_row || !rep_row) return set_err(GIQL_ERR_INVALID, "output buffer is NULL");
  if (n_chrom == 0) return set_err(GIQL_ERR_CHROM, "rows but n_chrom = 0");
  const size_t n = (size_t)s->n;
  LinBufs lb;
  SortBufs sb;
  OsScratch os;
  u32 *flags = nullptr, *excl = nullptr, *dummy_irr = nullptr;
  u64 *bsums = nullptr, *total = nullptr;
  auto carve = [&](char* base) {
    Carver c{base};
    common_sizes(c, n_chrom, lb);
    sort_sizes(c, n, sb, true);
    os_scratch_sizes(c, n, os);
    flags = c.take<u32>(n);
    excl = c.take<u32>(n + 1);
    bsums = c.take<u64>(cdiv((u64)n, SCAN_TILE) + 1);
    total = c.take<u64>(1);
    dummy_irr = c.take<u32>(16);
    return c.off;
  };
  GIQL_TRY(claim_arena(ctx, st, carve));
  giql_side raw = *s;  // identical RAW coordinates are what GROUP BY compares
  raw.start_off = raw.end_off = 0;
  giql_side none;
  memset(&none, 0, sizeof(none));
  const bool two_sorts = ctx->guess.nearest_two_sorts;
  GIQL_TRY(run_spans(ctx, st, raw, none, n_chrom, lb));
  GIQL_TRY(run_linearize(ctx, st, raw, n_chrom, lb, Side::A, LinTarget::keys_ends(sb.key[0], sb.end[0], dummy_irr),
                         LinOptions().keeping_irregular().counting_starts(os.starts())
                             .counting_ends(two_sorts ? os.ends() : DigitCounts())));
  if (two_sorts) {
    GIQL_TRY(run_sort_two_keys(ctx, st, sb, (u32)n, os));  // (start, end) order
  } else {
    GIQL_TRY(run_sort_onesweep(ctx, st, sb, sort_by_start(os, n)));
    Phase ph(ctx, st, GIQL_PH_AUX);
    hipLaunchKernelGGL(k_fix_start_ties, dim3(cdiv(n, 256)), dim3(256), 0, st, sb.key[0], sb.end[0],
                       sb.rid[0], (u32)n, ctx->d_meta);
  }
  {
    Phase ph(ctx, st, GIQL_PH_COUNT);
    hipLaunchKernelGGL(k_group_flags, dim3(cdiv(n, 256)), dim3(256), 0, st, sb.key[0], sb.end[0], (u32)n,
                       flags);
    GIQL_TRY(post_launch("group flags"));
  }
  GIQL_TRY(run_scan<u32>(ctx, st, GIQL_PH_SCAN, flags, (u64)n, excl, bsums, total));
  {
    Phase ph(ctx, st, GIQL_PH_FILL);
    hipLaunchKernelGGL(k_group_ids, dim3(cdiv(n, 256)), dim3(256), 0, st, sb.rid[0], flags, excl, (u32)n,
                       group_of_row, rep_row);
    GIQL_TRY(post_launch("group ids"));
  }
  u64 h_total = 0;
  HIP_TRY(hipMemcpyAsync(&h_total, total, sizeof(u64), hipMemcpyDeviceToHost, st));
  GIQL_TRY(read_meta(ctx, st));
  if (!two_sorts && ctx->h_meta->aux0 != 0) {  // a long run of equal starts: two-sort plan
    ctx->guess.nearest_two_sorts = true;
    return GIQL_STATUS_GUESS_MISSED;
  }
  collect_spans(ctx);
  *n_groups = (int64_t)h_total;
  ctx->stats.n_out = (int64_t)h_total;
  return GIQL_OK;
}

int giql_hip_group_rows_dev(giql_hip_ctx* ctx, const giql_side* s, int32_t n_chrom, int32_t* group_of_row,
                            int32_t* rep_row, int64_t* n_groups, void* stream) {
  return with_order_fallback(ctx, [&] {
    return giql_hip_group_rows_dev_impl(ctx, s, n_chrom, group_of_row, rep_row, n_groups, stream);
  });
}

int giql_hip_segment_sum_dev(giql_hip_ctx* ctx, const int64_t* values, const int32_t* group_of_row,
                             int64_t n, int64_t* sums, int64_t n_groups, void* stream) {
  if (!ctx || n < 0 || n_groups < 0 || n_groups > 0x7FFFFFFFll) return set_err(GIQL_ERR_INVALID, "bad arguments");
  if ((n > 0 && (!values || !group_of_row)) || (n_groups > 0 && !sums))
    return set_err(GIQL_ERR_INVALID, "NULL buffer");
  GIQL_TRY(begin_call_beside_plan(ctx));
  hipStream_t st = (hipStream_t)stream;
  if (n_groups > 0) HIP_TRY(hipMemsetAsync(sums, 0, (size_t)n_groups * sizeof(int64_t), st));
  if (n == 0) return GIQL_OK;
  HIP_TRY(hipMemsetAsync(&ctx->d_meta->status, 0, sizeof(int), st));
  u32 grid = cdiv((u64)n, 256 * 8);
  if (grid > GIQL_STREAM_GRID) grid = GIQL_STREAM_GRID;
  {
    Phase ph(ctx, st, GIQL_PH_AUX);
    hipLaunchKernelGGL(k_segment_sum, dim3(grid), dim3(256), 0, st, (const i64*)values, group_of_row, (u64)n,
                       (u32)n_groups, (unsigned long long*)sums, ctx->d_meta);
    GIQL_TRY(post_launch("segment sum"));
  }
  GIQL_TRY(read_meta(ctx, st));
  collect_spans(ctx);
  return GIQL_OK;
}

// -------------------------------------------------------------------- spans
int giql_hip_chrom_spans_dev(giql_hip_ctx* ctx, const giql_side* a, const giql_side* b,
                             int32_t n_chrom, int64_t* spans_out, void* stream) {
  if (!ctx || !spans_out) return set_err(GIQL_ERR_INVALID, "ctx/spans_out is NULL");
  GIQL_TRY(check_side(a, "a"));
  GIQL_TRY(check_side(b, "b"));
  if (n_chrom <= 0) return set_err(GIQL_ERR_INVALID, "n_chrom <= 0");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  LinBufs lb;
  auto carve = [&](char* base) {
    Carver c{base};
    common_sizes(c, n_chrom, lb);
    return c.off;
  };
  GIQL_TRY(claim_arena(ctx, st, carve));
  GIQL_TRY(run_spans(ctx, st, *a, *b, n_chrom, lb));
  std::vector<int> mn((size_t)n_chrom), mx((size_t)n_chrom);
  HIP_TRY(hipMemcpyAsync(mn.data(), lb.gmin, (size_t)n_chrom * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(mx.data(), lb.gmax, (size_t)n_chrom * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(ctx->h_meta, ctx->d_meta, sizeof(DevMeta), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (ctx->h_meta->status == GIQL_ERR_CHROM)
    return set_err(GIQL_ERR_CHROM, "a chrom id is outside [0, n_chrom)");
  int omin = a->start_off, omax = a->start_off;
  const int offs[3] = {a->end_off, b->start_off, b->end_off};
  for (int k = 0; k < 3; k++) {
    if (offs[k] < omin) omin = offs[k];
    if (offs[k] > omax) omax = offs[k];
  }
  for (int c = 0; c < n_chrom; c++)
    spans_out[c] = mn[c] <= mx[c] ? ((int64_t)mx[c] + omax) - ((int64_t)mn[c] + omin) + 1 : 0;
  return GIQL_OK;
}

// ---------------------------------------------------------------- checksum
int giql_hip_pairs_checksum_dev(giql_hip_ctx* ctx, const int32_t* row_a, const int32_t* row_b,
                                int64_t n, void* stream, uint64_t* out) {
  if (!ctx || !out || n < 0) return set_err(GIQL_ERR_INVALID, "bad arguments");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(ctx->d_scratch64, 0, sizeof(u64), st));
  if (n > 0) {
    u32 grid = cdiv((u64)n, 256 * 8);
    if (grid > GIQL_STREAM_GRID) grid = GIQL_STREAM_GRID;
    hipLaunchKernelGGL(k_pairs_checksum, dim3(grid), dim3(256), 0, st, row_a, row_b, (u64)n,
                       ctx->d_scratch64);
    GIQL_TRY(post_launch("checksum"));
  }
  u64 h = 0;
  HIP_TRY(hipMemcpyAsync(&h, ctx->d_scratch64, sizeof(u64), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  *out = h;
  return GIQL_OK;
}


// ------------------------------------------- compact plan (multi-GPU exchange)
// The uniform-length plan IS a compact description of the result: per query row its id, the
// first matching position in the other side's sorted order and the number of matches, plus
// that side's row ids in sorted order -- 12 B per query row + 4 B per row instead of 8 B per
// pair (65 MB instead of 400 MB per rank at BASELINE config 4 on 8 GPUs).  Ranks exchange THAT
// and every receiver expands it with the same partition + fill kernels the local join uses.
// (the counts come from the offsets: the fused count leaves upper bounds, not counts, in the plan's cnt array)
__global__ __launch_bounds__(256) void k_plan_export(const u32* __restrict__ q_rid, const u32* __restrict__ lo,
                                                      const u64* __restrict__ off, u32 n_q,
                                                      const u32* __restrict__ s_rid, u32 n_s, u32 q_add, u32 s_add,
                                                      int32_t* __restrict__ q_rid_out, u32* __restrict__ lo_out,
                                                      u32* __restrict__ cnt_out, int32_t* __restrict__ s_rid_out) {
  const u64 stride = (u64)gridDim.x * 256;
  for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < (u64)n_q + n_s; i += stride) {
    if (i < n_q) {
      q_rid_out[i] = (int32_t)(q_rid[i] + q_add);
      lo_out[i] = lo[i];
      cnt_out[i] = (u32)(off[i + 1] - off[i]);
    } else {
      const u64 j = i - n_q;
      s_rid_out[j] = (int32_t)(s_rid[j] + s_add);
    }
  }
}

int giql_hip_inner_plan_export_dev(giql_hip_ctx* ctx, int32_t* q_rid_out, uint32_t* lo_out, uint32_t* cnt_out,
                                   int32_t* s_rid_out, int64_t q_capacity, int64_t s_capacity,
                                   int32_t rid_add_a, int32_t rid_add_b, int32_t* query_is_a, int64_t* n_q,
                                   int64_t* n_s, void* stream) {
  if (!ctx || !query_is_a || !n_q || !n_s) return set_err(GIQL_ERR_INVALID, "NULL argument");
  if (ctx->kept != Plan::INNER) return set_err(GIQL_ERR_STATE, "plan export without a successful inner_plan");
  if (ctx->plan.plan_is_join && ctx->plan.n_reg + ctx->plan.n_irr != 0)
    return set_err(GIQL_ERR_STATE, "the last giql_hip_inner_join_dev wrote its pairs itself and kept no plan: "
                                   "call giql_hip_inner_plan_dev first");
  InnerState& S = ctx->plan.inner;
  const bool empty = ctx->plan.n_reg + ctx->plan.n_irr == 0;
  if (!empty && (S.uniform == 0 || ctx->plan.n_irr != 0 || ctx->plan.n_c1 != 0))
    return set_err(GIQL_ERR_STATE, "the last plan is not in the compact single-range form "
                                   "(general two-class join or irregular rows): exchange the pairs instead");
  const bool q_is_a = S.uniform != 2;  // in the plan's labels
  *query_is_a = (q_is_a != ctx->plan.swapped) ? 1 : 0;
  if (ctx->plan.swapped) {
    const int32_t t = rid_add_a;
    rid_add_a = rid_add_b;
    rid_add_b = t;
  }
  *n_q = empty ? 0 : (q_is_a ? ctx->plan.n_a : ctx->plan.n_b);
  *n_s = empty ? 0 : (q_is_a ? ctx->plan.n_b : ctx->plan.n_a);
  if (empty) return GIQL_OK;
  if (*n_q > q_capacity || *n_s > s_capacity)
    return set_err(GIQL_ERR_CAPACITY, "plan export needs %lld query rows and %lld sorted rows", (long long)*n_q,
                   (long long)*n_s);
  if (!q_rid_out || !lo_out || !cnt_out || !s_rid_out) return set_err(GIQL_ERR_INVALID, "NULL output");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const u32* qrid = q_is_a ? S.sa.rid[0] : S.sb.rid[0];
  const u32* srid = q_is_a ? S.sb.rid[0] : S.sa.rid[0];
  u32 grid = cdiv((u64)(*n_q + *n_s), 256 * 8);
  if (grid > GIQL_STREAM_GRID) grid = GIQL_STREAM_GRID;
  hipLaunchKernelGGL(k_plan_export, dim3(grid), dim3(256), 0, st, qrid, S.lo2, S.off2, (u32)*n_q, srid, (u32)*n_s,
                     (u32)(q_is_a ? rid_add_a : rid_add_b), (u32)(q_is_a ? rid_add_b : rid_add_a), q_rid_out,
                     lo_out, cnt_out, s_rid_out);
  return post_launch("plan export");
}

int giql_hip_fill_from_plan_dev(giql_hip_ctx* ctx, const int32_t* q_rid, const uint32_t* lo, const uint32_t* cnt,
                                int64_t n_q, const int32_t* s_rid, int64_t n_s, int32_t* row_q, int32_t* row_s,
                                int64_t capacity, int64_t n_pairs_expected, void* stream, int64_t* n_pairs) {
  if (!ctx || !n_pairs) return set_err(GIQL_ERR_INVALID, "ctx/n_pairs is NULL");
  if (n_q < 0 || n_q > 0x7FFFFFF0ll || n_s < 0 || n_s > 0x7FFFFFF0ll || capacity < 0)
    return set_err(GIQL_ERR_INVALID, "bad sizes");
  *n_pairs = 0;
  if (n_q == 0 || n_s == 0) return GIQL_OK;
  if (!q_rid || !lo || !cnt || !s_rid) return set_err(GIQL_ERR_INVALID, "NULL plan array");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  constexpr u32 T2 = FILL_NT * FILL_ITEMS_C2;
  // scratch: exclusive u64 offsets [n_q + 1], scan partials, partition array for `capacity` pairs
  const u64 nt_cap = ((u64)capacity + T2 - 1) / T2;
  if (nt_cap > 0x7FFFFFF0ull) return set_err(GIQL_ERR_INVALID, "output too large");
  u64* off = nullptr;
  u64* bsums = nullptr;
  u32* part = nullptr;
  auto carve = [&](char* base) {
    Carver c{base};
    off = c.take<u64>((size_t)n_q + 1);
    bsums = c.take<u64>(cdiv((u64)n_q, SCAN_TILE) + 2);
    part = c.take<u32>((size_t)nt_cap + 2);
    return c.off;
  };
  const size_t need = carve(nullptr);
  GIQL_TRY(ctx->xplan.grow(need, align_up(need + need / 8, (size_t)1 << 20), st, "the plan scratch"));
  carve(ctx->xplan);
  GIQL_TRY(run_scan<u64>(ctx, st, GIQL_PH_SCAN, cnt, (u64)n_q, off, bsums, off + n_q));
  u64 total = 0;
  if (n_pairs_expected >= 0) {
    total = (u64)n_pairs_expected;  // the caller knows it (all-gathered counts): no read-back, no stream sync
  } else {
    HIP_TRY(hipMemcpyAsync(&total, off + n_q, sizeof(u64), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  *n_pairs = (int64_t)total;
  if (total == 0) return GIQL_OK;
  if (total > (u64)capacity)
    return set_err(GIQL_ERR_CAPACITY, "capacity %lld < %llu pairs", (long long)capacity, (unsigned long long)total);
  if (!row_q || !row_s) return set_err(GIQL_ERR_INVALID, "row_q/row_s is NULL");
  const u32 nt = (u32)((total + T2 - 1) / T2);
  {
    Phase ph(ctx, st, GIQL_PH_PARTITION);
    hipLaunchKernelGGL(k_partition, dim3(cdiv((u64)nt + 1, 256)), dim3(256), 0, st, off, (u32)n_q, (u64)0, T2, nt,
                       part, (const u64*)(off + n_q), (u64)capacity);
  }
  {
    // the pair count is read on the device (off[n_q]): a wrong n_pairs_expected cannot overrun
    Phase ph(ctx, st, GIQL_PH_FILL);
    hipLaunchKernelGGL((k_fill<FILL_ITEMS_C2>), dim3(nt), dim3(FILL_NT), 0, st, off, lo,
                       reinterpret_cast<const u32*>(q_rid), (u32)n_q, reinterpret_cast<const u32*>(s_rid), part,
                       (u64)0, (u64)0, row_q, row_s, (const u64*)(off + n_q), (u64)capacity);
  }
  return post_launch("fill from plan");
}

// ------------------------------------------------------------ copy probe
// The box's own streaming-copy rate with THIS library's access pattern (16 B per lane, grid-
// stride): the yardstick bench.py reports next to the 8 TB/s peak.
__global__ __launch_bounds__(256) void k_copy16(const uint4* __restrict__ src, uint4* __restrict__ dst, u64 n16) {
  const u64 stride = (u64)gridDim.x * 256;
  for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n16; i += stride) dst[i] = src[i];
}

int giql_hip_copy_probe_dev(giql_hip_ctx* ctx, const void* src, void* dst, int64_t bytes, int32_t reps,
                            void* stream, double* gbytes_per_s) {
  if (!ctx || !src || !dst || !gbytes_per_s || bytes < 16 || reps < 1) return set_err(GIQL_ERR_INVALID, "bad arguments");
  if (((uintptr_t)src | (uintptr_t)dst) & 15) return set_err(GIQL_ERR_INVALID, "buffers must be 16-byte aligned");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const u64 n16 = (u64)bytes / 16;
  const u32 grid = (u32)ctx->n_cu * 8;  // one resident wave of 256-thread blocks
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  hipLaunchKernelGGL(k_copy16, dim3(grid), dim3(256), 0, st, (const uint4*)src, (uint4*)dst, n16);  // warm-up
  (void)hipEventRecord(e0, st);
  for (int r = 0; r < reps; r++)
    hipLaunchKernelGGL(k_copy16, dim3(grid), dim3(256), 0, st, (const uint4*)src, (uint4*)dst, n16);
  (void)hipEventRecord(e1, st);
  hipError_t e = hipEventSynchronize(e1);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (e != hipSuccess) return set_err(GIQL_ERR_HIP, "copy probe failed: %s", hipGetErrorString(e));
  GIQL_TRY(post_launch("copy probe"));
  *gbytes_per_s = ms > 0.f ? 2.0 * (double)(n16 * 16) * reps / ((double)ms * 1e6) : 0.0;
  return GIQL_OK;
}

// The same question asked properly (round 4): what does this device read / write / copy per second, by access
// shape?  mode 0 read only, 1 write only, 2 copy, 3 hipMemcpyDtoDAsync (an outside reference); in_flight = 16-byte
// accesses a thread keeps in flight (1, 2, 4 or 8); nontemporal = nt loads and stores; blocks_per_cu sizes the grid
// (256-thread blocks).  *gbytes_per_s counts every byte moved: read for mode 0, written for 1, both for 2 / 3.
int giql_hip_stream_probe_dev(giql_hip_ctx* ctx, const void* src, void* dst, int64_t bytes, int32_t mode,
                              int32_t in_flight, int32_t nontemporal, int32_t blocks_per_cu, int32_t reps, void* stream,
                              double* gbytes_per_s) {
  if (!ctx || !src || !dst || !gbytes_per_s || bytes < (1 << 20) || reps < 1 || mode < 0 || mode > 3 ||
      blocks_per_cu < 1 || blocks_per_cu > 64 || (in_flight != 1 && in_flight != 2 && in_flight != 4 && in_flight != 8))
    return set_err(GIQL_ERR_INVALID, "bad arguments");
  if (((uintptr_t)src | (uintptr_t)dst) & 15) return set_err(GIQL_ERR_INVALID, "buffers must be 16-byte aligned");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const u64 tile = (u64)256 * (u64)in_flight;
  const u64 n16 = (u64)bytes / 16 / tile * tile;  // whole tiles only
  const u32 grid = (u32)ctx->n_cu * (u32)blocks_per_cu;
  auto once = [&]() {
    const probe_u4* s = (const probe_u4*)src;
    probe_u4* d = (probe_u4*)dst;
    u32* sk = ctx->bucket_qwin;  // the read-only form's sink (256 words, rewritten by every join that reads them)
    if (mode == 3) {
      (void)hipMemcpyDtoDAsync((hipDeviceptr_t)dst, (hipDeviceptr_t)src, n16 * 16, st);
    } else if (nontemporal) {
      if (mode == 0) launch_stream_probe<0, true>(in_flight, grid, st, s, d, n16, sk);
      else if (mode == 1) launch_stream_probe<1, true>(in_flight, grid, st, s, d, n16, sk);
      else launch_stream_probe<2, true>(in_flight, grid, st, s, d, n16, sk);
    } else {
      if (mode == 0) launch_stream_probe<0, false>(in_flight, grid, st, s, d, n16, sk);
      else if (mode == 1) launch_stream_probe<1, false>(in_flight, grid, st, s, d, n16, sk);
      else launch_stream_probe<2, false>(in_flight, grid, st, s, d, n16, sk);
    }
  };
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  once();  // warm-up
  (void)hipEventRecord(e0, st);
  for (int r = 0; r < reps; r++) once();
  (void)hipEventRecord(e1, st);
  hipError_t e = hipEventSynchronize(e1);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (e != hipSuccess) return set_err(GIQL_ERR_HIP, "stream probe failed: %s", hipGetErrorString(e));
  GIQL_TRY(post_launch("stream probe"));
  const double moved = (mode >= 2 ? 2.0 : 1.0) * (double)(n16 * 16) * reps;
  *gbytes_per_s = ms > 0.f ? moved / ((double)ms * 1e6) : 0.0;
  return GIQL_OK;
}

// ------------------------------------------------ projection (Arrow take)
int giql_hip_take_dev(giql_hip_ctx* ctx, const void* const* cols, const int32_t* elem_bytes,
                      int32_t n_cols, int64_t n_rows, const int32_t* idx, int64_t n,
                      void* const* outs, void* stream) {
  if (!ctx || n_cols < 0 || n < 0 || n_rows < 0 || n_rows > 0x7FFFFFFFll || (n_cols && (!cols || !elem_bytes || !outs)))
    return set_err(GIQL_ERR_INVALID, "bad arguments");
  if (n > 0 && !idx) return set_err(GIQL_ERR_INVALID, "idx is NULL");
  for (int c = 0; c < n_cols; c++) {
    const int e = elem_bytes[c];
    if (e != 1 && e != 2 && e != 4 && e != 8 && e != 16)
      return set_err(GIQL_ERR_INVALID, "column %d: elem_bytes=%d not in {1,2,4,8,16}", c, e);
    if (n > 0 && (!outs[c] || (n_rows > 0 && !cols[c])))
      return set_err(GIQL_ERR_INVALID, "column %d: NULL buffer", c);
    if (((uintptr_t)cols[c] | (uintptr_t)outs[c]) % (uintptr_t)e)
      return set_err(GIQL_ERR_INVALID, "column %d: buffer not aligned to its element size", c);
  }
  if (n == 0 || n_cols == 0) return GIQL_OK;
  GIQL_TRY(begin_call_beside_plan(ctx));
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(&ctx->d_meta->status, 0, sizeof(int), st));
  u32 grid = cdiv((u64)n, (u64)TK_NT * 4 * 4);
  if (grid > GIQL_STREAM_GRID) grid = GIQL_STREAM_GRID;
  for (int c0 = 0; c0 < n_cols; c0 += TK_MAX_COLS) {
    TakeArgs a;
    memset(&a, 0, sizeof(a));
    a.n_cols = n_cols - c0 < TK_MAX_COLS ? n_cols - c0 : TK_MAX_COLS;
    a.vec = ((uintptr_t)idx % 16) == 0;
    for (int c = 0; c < a.n_cols; c++) {
      a.col[c] = cols[c0 + c];
      a.out[c] = outs[c0 + c];
      a.elem[c] = elem_bytes[c0 + c];
      if ((uintptr_t)a.out[c] % 16) a.vec = 0;
    }
    Phase ph(ctx, st, GIQL_PH_AUX);
    hipLaunchKernelGGL(k_take, dim3(grid), dim3(TK_NT), 0, st, a, idx, (u64)n, (u32)n_rows,
                       ctx->d_meta);
    GIQL_TRY(post_launch("take"));
  }
  GIQL_TRY(read_meta(ctx, st));
  collect_spans(ctx);
  ctx->stats.n_out = n;
  return GIQL_OK;
}

int giql_hip_take_utf8_plan_dev(giql_hip_ctx* ctx, const int32_t* offsets, int64_t n_rows,
                                const int32_t* idx, int64_t n, int32_t* out_offsets,
                                int64_t* n_bytes, void* stream) {
  if (!ctx || !out_offsets || !n_bytes || n < 0 || n > 0x7FFFFFF0ll || n_rows < 0 || n_rows > 0x7FFFFFFFll)
    return set_err(GIQL_ERR_INVALID, "bad arguments");
  if ((n > 0 && !idx) || (n_rows > 0 && !offsets)) return set_err(GIQL_ERR_INVALID, "NULL buffer");
  GIQL_TRY(begin_call(ctx));
  hipStream_t st = (hipStream_t)stream;
  *n_bytes = 0;
  if (n == 0) {
    HIP_TRY(hipMemsetAsync(out_offsets, 0, sizeof(int32_t), st));
    HIP_TRY(hipStreamSynchronize(st));
    return GIQL_OK;
  }
  u64 *bsums = nullptr, *total = nullptr;
  GIQL_TRY(claim_arena(ctx, st, [&](char* base) {
    Carver c{base};
    bsums = c.take<u64>(cdiv((u64)n, SCAN_TILE) + 1);
    total = c.take<u64>(1);
    return c.off;
  }));
  HIP_TRY(hipMemsetAsync(&ctx->d_meta->status, 0, sizeof(int), st));
  u32 grid = cdiv((u64)n, (u64)TK_NT * 4);
  if (grid > GIQL_STREAM_GRID) grid = GIQL_STREAM_GRID;
  {
    Phase ph(ctx, st, GIQL_PH_AUX);
    hipLaunchKernelGGL(k_take_utf8_len, dim3(grid), dim3(TK_NT), 0, st, offsets, (u32)n_rows, idx,
                       (u64)n, reinterpret_cast<u32*>(out_offsets), ctx->d_meta);
    GIQL_TRY(post_launch("take_utf8_len"));
  }
  GIQL_TRY(run_scan<u32>(ctx, st, GIQL_PH_SCAN, reinterpret_cast<u32*>(out_offsets), (u64)n,
                         reinterpret_cast<u32*>(out_offsets), bsums, total));
  // out_offsets[n] = total (low word; the range check below rejects anything wider)
  HIP_TRY(hipMemcpyAsync(out_offsets + n, total, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  u64 h_total = 0;
  HIP_TRY(hipMemcpyAsync(&h_total, total, sizeof(u64), hipMemcpyDeviceToHost, st));
  GIQL_TRY(read_meta(ctx, st));
  collect_spans(ctx);
  if (h_total > 0x7FFFFFFFull)
    return set_err(GIQL_ERR_CAPACITY, "taken utf8 data is %llu bytes: exceeds int32 offsets",
                   (unsigned long long)h_total);
  *n_bytes = (int64_t)h_total;
  return GIQL_OK;
}

int giql_hip_take_utf8_fill_dev(giql_hip_ctx* ctx, const int32_t* offsets, const uint8_t* data,
                                int64_t n_rows, const int32_t* idx, int64_t n,
                                const int32_t* out_offsets, uint8_t* out_data, void* stream) {
  if (!ctx || n < 0 || n_rows < 0 || n_rows > 0x7FFFFFFFll) return set_err(GIQL_ERR_INVALID, "bad arguments");
  if (n == 0) return GIQL_OK;
  if (!idx || !out_offsets || (n_rows > 0 && !offsets)) return set_err(GIQL_ERR_INVALID, "NULL buffer");
  GIQL_TRY(begin_call_beside_plan(ctx));
  hipStream_t st = (hipStream_t)stream;
  u32 grid = cdiv((u64)n, (u64)TK_NT * 2);
  if (grid > 2u * GIQL_STREAM_GRID) grid = 2u * GIQL_STREAM_GRID;
  {
    Phase ph(ctx, st, GIQL_PH_AUX);
    hipLaunchKernelGGL(k_take_utf8_copy, dim3(grid), dim3(TK_NT), 0, st, offsets, data, (u32)n_rows,
                       idx, (u64)n, out_offsets, out_data);
    GIQL_TRY(post_launch("take_utf8_copy"));
  }
  HIP_TRY(hipStreamSynchronize(st));
  collect_spans(ctx);
  ctx->stats.n_out = n;
  return GIQL_OK;
}

// ------------------------------------------------ residual predicates (select)
static int check_operand(const giql_operand& o, int k, const char* which, const char* owner) {
  if (o.side == GIQL_SIDE_LIT) return GIQL_OK;
  if (o.side != GIQL_SIDE_A && o.side != GIQL_SIDE_B)
    return set_err(GIQL_ERR_INVALID, "%s %d %s: side %d", owner, k, which, o.side);
  if (o.type < GIQL_T_I32 || o.type > GIQL_T_U8)
    return set_err(GIQL_ERR_INVALID, "%s %d %s: type %d", owner, k, which, o.type);
  if (!o.data) return set_err(GIQL_ERR_INVALID, "%s %d %s: NULL column", owner, k, which);
  return GIQL_OK;
}

int giql_hip_select_dev(giql_hip_ctx* ctx, const giql_pred* preds, int32_t n_preds,
                        const int32_t* idx_a, int64_t n_rows_a, const int32_t* idx_b,
                        int64_t n_rows_b, int64_t n, int32_t* out_a, int32_t* out_b,
                        int64_t* n_kept, void* stream) {
  return giql_hip_select_expr_dev(ctx, preds, n_preds, nullptr, 0, idx_a, n_rows_a, idx_b, n_rows_b, n, out_a, out_b,
                                  n_kept, stream);
}

int giql_hip_select_expr_dev(giql_hip_ctx* ctx, const giql_pred* preds, int32_t n_preds,
                             const giql_operand* nodes, int32_t n_nodes,
                             const int32_t* idx_a, int64_t n_rows_a, const int32_t* idx_b,
                             int64_t n_rows_b, int64_t n, int32_t* out_a, int32_t* out_b,
                             int64_t* n_kept, void* stream) {
  if (!ctx || !n_kept || n < 0 || n > 0x7FFFFFF0ll || n_preds < 0 || n_preds > SEL_MAX_PREDS ||
      (n_preds && !preds) || n_rows_a < 0 || n_rows_b < 0 || n_rows_a > 0x7FFFFFFFll ||
      n_rows_b > 0x7FFFFFFFll || n_nodes < 0 || n_nodes > SEL_MAX_NODES || (n_nodes && !nodes))
    return set_err(GIQL_ERR_INVALID, "bad arguments (at most %d predicates and %d expression nodes, n < 2^31)",
                   SEL_MAX_PREDS, SEL_MAX_NODES);
  static_assert(GIQL_SIDE_EXPR == SEL_SIDE_EXPR && GIQL_X_ADD == SEL_X_ADD && GIQL_X_GREATEST == SEL_X_GREATEST &&
                GIQL_X_NEG == SEL_X_NEG && GIQL_X_ABS == SEL_X_ABS && GIQL_X_DIV == SEL_X_DIV &&
                GIQL_X_EQ == SEL_X_EQ && GIQL_X_NOT == SEL_X_NOT && GIQL_X_IF == SEL_X_IF && GIQL_X_NULL == SEL_X_NULL,
                "expression node kinds");
  DevPreds ps;
  bool uses[2] = {false, false};
  bool any_expr = false;
  GIQL_TRY(convert_preds(preds, n_preds, ps, uses, nodes, n_nodes, &any_expr));
  // a side given neither ids nor a row count is addressed by the candidate index
  if (!idx_a && n_rows_a == 0 && !uses[0]) n_rows_a = n;
  if (!idx_b && n_rows_b == 0 && !uses[1]) n_rows_b = n;
  *n_kept = 0;
  GIQL_TRY(begin_call(ctx));  // (before the way out with no candidates: that one drops a plan too)
  if (n == 0) return GIQL_OK;
  hipStream_t st = (hipStream_t)stream;
  const u32 nb = cdiv((u64)n, SEL_TILE);
  DevOperand* prog = nullptr;
  u64 *mask = nullptr, *bsums = nullptr, *total = nullptr;
  u32* cnt = nullptr;
  GIQL_TRY(claim_arena(ctx, st, [&](char* base) {
    Carver c{base};
    mask = c.take<u64>(((size_t)n + 63) / 64);
    cnt = c.take<u32>(nb);
    bsums = c.take<u64>(cdiv((u64)nb, SCAN_TILE) + 1);
    total = c.take<u64>(1);
    prog = c.take<DevOperand>(SEL_MAX_NODES);
    return c.off;
  }));
  HIP_TRY(hipMemsetAsync(&ctx->d_meta->status, 0, sizeof(int), st));
  if (any_expr)  // (pageable source: staged by the runtime before the call returns)
    HIP_TRY(hipMemcpyAsync(prog, nodes, (size_t)n_nodes * sizeof(DevOperand), hipMemcpyHostToDevice, st));
  {
    Phase ph(ctx, st, GIQL_PH_COUNT);
    if (any_expr)
      hipLaunchKernelGGL((k_select_count<true>), dim3(nb), dim3(SEL_NT), 0, st, ps, (const DevOperand*)prog, idx_a,
                         (u32)n_rows_a, idx_b, (u32)n_rows_b, (u64)n, mask, cnt, ctx->d_meta);
    else
      hipLaunchKernelGGL((k_select_count<false>), dim3(nb), dim3(SEL_NT), 0, st, ps, (const DevOperand*)nullptr, idx_a,
                         (u32)n_rows_a, idx_b, (u32)n_rows_b, (u64)n, mask, cnt, ctx->d_meta);
    GIQL_TRY(post_launch("select_count"));
  }
  GIQL_TRY(run_scan<u32>(ctx, st, GIQL_PH_SCAN, cnt, (u64)nb, cnt, bsums, total));
  if (out_a || out_b) {
    Phase ph(ctx, st, GIQL_PH_FILL);
    hipLaunchKernelGGL(k_select_scatter, dim3(nb), dim3(SEL_NT), 0, st, idx_a, idx_b, (u64)n, mask, cnt,
                       out_a, out_b);
    GIQL_TRY(post_launch("select_scatter"));
  }
  u64 h_total = 0;
  HIP_TRY(hipMemcpyAsync(&h_total, total, sizeof(u64), hipMemcpyDeviceToHost, st));
  GIQL_TRY(read_meta(ctx, st));
  collect_spans(ctx);
  *n_kept = (int64_t)h_total;
  ctx->stats.n_out = (int64_t)h_total;
  return GIQL_OK;
}

// ------------------------------------------------ computed columns (eval)
// The value of up to EV_MAX_OUTS programs per candidate, in one pass (eval_kernels.hip.h).  The programs are checked
// and statically typed on the host before anything is launched; the nodes are staged in the arena like select's.
int giql_hip_eval_expr_dev(giql_hip_ctx* ctx, const giql_operand* nodes, int32_t n_nodes, const giql_expr_out* outs,
                           int32_t n_outs, const int32_t* idx_a, int64_t n_rows_a, const int32_t* idx_b,
                           int64_t n_rows_b, int64_t n, int64_t* n_null, void* stream) {
  if (!ctx || n < 0 || n > 0x7FFFFFF0ll || n_rows_a < 0 || n_rows_b < 0 || n_rows_a > 0x7FFFFFFFll ||
      n_rows_b > 0x7FFFFFFFll || n_nodes < 0 || n_nodes > SEL_MAX_NODES || (n_nodes && !nodes))
    return set_err(GIQL_ERR_INVALID, "bad arguments (at most %d expression nodes, n < 2^31)", SEL_MAX_NODES);
  if (n_outs < 1 || n_outs > EV_MAX_OUTS || !outs)
    return set_err(GIQL_ERR_INVALID, "n_outs = %d outside [1, %d]", n_outs, EV_MAX_OUTS);
  static_assert(sizeof(giql_expr_out) == sizeof(DevExprOut), "giql_expr_out layout");
  DevExprOuts d;
  memset(&d, 0, sizeof(d));
  d.n = n_outs;
  bool uses[2] = {false, false};
  for (int k = 0; k < n_outs; k++) {
    if (outs[k].type != GIQL_T_I64 && outs[k].type != GIQL_T_F64)
      return set_err(GIQL_ERR_INVALID, "output %d: type %d (GIQL_T_I64 or GIQL_T_F64)", k, outs[k].type);
    if (n > 0 && !outs[k].data) return set_err(GIQL_ERR_INVALID, "output %d: data is NULL", k);
    bool can_float = false;
    GIQL_TRY(check_program(nodes, n_nodes, outs[k].first, outs[k].count, k, "program", uses, "output", &can_float));
    if (can_float && outs[k].type == GIQL_T_I64)
      return set_err(GIQL_ERR_INVALID, "output %d: the program can yield a float, its output is GIQL_T_I64", k);
    memcpy(&d.o[k], &outs[k], sizeof(DevExprOut));
  }
  // a side given neither ids nor a row count is addressed by the candidate index
  if (!idx_a && n_rows_a == 0 && !uses[0]) n_rows_a = n;
  if (!idx_b && n_rows_b == 0 && !uses[1]) n_rows_b = n;
  if (n_null) memset(n_null, 0, (size_t)n_outs * sizeof(int64_t));
  GIQL_TRY(begin_call(ctx));  // (before the way out with no candidates: that one drops a plan too)
  if (n == 0) return GIQL_OK;
  hipStream_t st = (hipStream_t)stream;
  DevOperand* prog = nullptr;
  u64* nulls = nullptr;
  GIQL_TRY(claim_arena(ctx, st, [&](char* base) {
    Carver c{base};
    prog = c.take<DevOperand>(SEL_MAX_NODES);
    nulls = c.take<u64>(EV_MAX_OUTS);
    return c.off;
  }));
  HIP_TRY(hipMemsetAsync(&ctx->d_meta->status, 0, sizeof(int), st));
  HIP_TRY(hipMemsetAsync(nulls, 0, EV_MAX_OUTS * sizeof(u64), st));
  // (pageable source: staged by the runtime before the call returns)
  HIP_TRY(hipMemcpyAsync(prog, nodes, (size_t)n_nodes * sizeof(DevOperand), hipMemcpyHostToDevice, st));
  const u32 n_tiles = cdiv((u64)n, SEL_TILE);
  {
    Phase ph(ctx, st, GIQL_PH_AUX);
    ctx->stats.phase_bytes[GIQL_PH_AUX] += (int64_t)(8 + 9 * n_outs) * n;  // ids read, 8 B + 1 B per output (+ the gathers)
    hipLaunchKernelGGL(k_eval_expr, dim3(n_tiles < GIQL_STREAM_GRID ? n_tiles : GIQL_STREAM_GRID), dim3(SEL_NT), 0, st, d,
                       (const DevOperand*)prog, idx_a, (u32)n_rows_a, idx_b, (u32)n_rows_b, (u64)n, n_tiles, nulls,
                       ctx->d_meta);
    GIQL_TRY(post_launch("eval_expr"));
  }
  u64 h_nulls[EV_MAX_OUTS] = {0};
  HIP_TRY(hipMemcpyAsync(h_nulls, nulls, sizeof(h_nulls), hipMemcpyDeviceToHost, st));
  if (read_meta(ctx, st) != GIQL_OK) {
    if (ctx->h_meta->status == GIQL_ERR_INVALID) return set_err(GIQL_ERR_INVALID, "a row id is outside its table");
    return ctx->h_meta->status ? ctx->h_meta->status : GIQL_ERR_HIP;
  }
  collect_spans(ctx);
  if (n_null)
    for (int k = 0; k < n_outs; k++) n_null[k] = (int64_t)h_nulls[k];
  ctx->stats.n_out = n;
  return GIQL_OK;
}

int giql_hip_mark_dev(giql_hip_ctx* ctx, const int32_t* idx, int64_t n, uint8_t* flags,
                      int64_t n_rows, void* stream) {
  if (!ctx || n < 0 || n_rows < 0 || n_rows > 0x7FFFFFFFll || (n > 0 && (!idx || !flags)))
    return set_err(GIQL_ERR_INVALID, "bad arguments");
  if (n == 0) return GIQL_OK;
  GIQL_TRY(begin_call_beside_plan(ctx));
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(&ctx->d_meta->status, 0, sizeof(int), st));
  u32 grid = cdiv((u64)n, 256 * 8);
  if (grid > GIQL_STREAM_GRID) grid = GIQL_STREAM_GRID;
  {
    Phase ph(ctx, st, GIQL_PH_AUX);
    hipLaunchKernelGGL(k_mark, dim3(grid), dim3(256), 0, st, idx, (u64)n, (u32)n_rows, flags, ctx->d_meta);
    GIQL_TRY(post_launch("mark"));
  }
  GIQL_TRY(read_meta(ctx, st));
  collect_spans(ctx);
  return GIQL_OK;
}

// ------------------------------------------------- literal range sets (ANY)
// The sets' tables are prepared on the host (range_set_prepare.h), laid out in one block of the arena and copied in
// one transfer; one launch answers every set (grid.y = set).
int giql_hip_range_set_any_dev(giql_hip_ctx* ctx, const int32_t* chrom, const int32_t* start, const int32_t* end,
                               const uint8_t* valid_chrom, const uint8_t* valid_start, const uint8_t* valid_end,
                               int64_t n, const giql_range_set* sets, int32_t n_sets, void* stream) {
  static_assert(GIQL_RANGE_INTERSECTS == RSET_INTERSECTS && GIQL_RANGE_CONTAINS == RSET_CONTAINS &&
                GIQL_RANGE_WITHIN == RSET_WITHIN && GIQL_RANGE_MAX_SETS == RSET_MAX_SETS &&
                GIQL_RANGE_MAX_RANGES == RSET_MAX_RANGES, "range set constants");
  if (!ctx || n < 0 || n > 0x7FFFFFF0ll || !sets || n_sets < 1 || n_sets > RSET_MAX_SETS ||
      (n > 0 && (!chrom || !start || !end)))
    return set_err(GIQL_ERR_INVALID, "bad arguments (1..%d sets, n in [0, 2^31-16], no NULL column)", RSET_MAX_SETS);
  for (int k = 0; k < n_sets; k++) {
    const giql_range_set& s = sets[k];
    if (s.op < RSET_INTERSECTS || s.op > RSET_WITHIN) return set_err(GIQL_ERR_INVALID, "range set %d: op %d", k, s.op);
    if (s.n_ranges < 1 || s.n_ranges > RSET_MAX_RANGES)
      return set_err(GIQL_ERR_INVALID, "range set %d: %d ranges outside [1, %d]", k, s.n_ranges, RSET_MAX_RANGES);
    if (!s.chrom || !s.on_start || !s.on_end || (n > 0 && (!s.out_value || !s.out_valid)))
      return set_err(GIQL_ERR_INVALID, "range set %d: NULL array", k);
  }
  GIQL_TRY(begin_call(ctx, n));  // (before the way out with no rows: that one drops a plan too)
  if (n == 0) return GIQL_OK;
  hipStream_t st = (hipStream_t)stream;
  // the block: per set chrom[k] (int32), then key / other / agg (int64), every array 16-byte aligned
  std::vector<char> blob;
  size_t off[RSET_MAX_SETS][4];
  size_t total = 0;
  for (int k = 0; k < n_sets; k++) {
    const size_t nr = (size_t)sets[k].n_ranges;
    off[k][0] = total;
    total = align_up(total + nr * sizeof(int32_t), 16);
    for (int a = 1; a < 4; a++) {
      off[k][a] = total;
      total = align_up(total + nr * sizeof(i64), 16);
    }
  }
  blob.resize(total);
  RangeSetTable t;
  for (int k = 0; k < n_sets; k++) {
    const giql_range_set& s = sets[k];
    if (!range_set_prepare(s.op, s.chrom, s.on_start, s.on_end, s.n_ranges, t))
      return set_err(GIQL_ERR_INVALID, "range set %d could not be prepared", k);
    const size_t nr = (size_t)s.n_ranges;
    memcpy(blob.data() + off[k][0], t.chrom.data(), nr * sizeof(int32_t));
    memcpy(blob.data() + off[k][1], t.key.data(), nr * sizeof(i64));
    memcpy(blob.data() + off[k][2], t.other.data(), nr * sizeof(i64));
    memcpy(blob.data() + off[k][3], t.agg.data(), nr * sizeof(i64));
  }
  char* d_blob = nullptr;
  GIQL_TRY(claim_arena(ctx, st, [&](char* base) {
    Carver c{base};
    d_blob = c.take<char>(total);
    return c.off;
  }));
  HIP_TRY(hipMemcpyAsync(d_blob, blob.data(), total, hipMemcpyHostToDevice, st));
  RsArgs args;
  memset(&args, 0, sizeof(args));
  uintptr_t a16 = (uintptr_t)chrom | (uintptr_t)start | (uintptr_t)end;
  uintptr_t a4 = (uintptr_t)valid_chrom | (uintptr_t)valid_start | (uintptr_t)valid_end;
  for (int k = 0; k < n_sets; k++) {
    RsSetDev& d = args.set[k];
    d.chrom = reinterpret_cast<const int32_t*>(d_blob + off[k][0]);
    d.key = reinterpret_cast<const i64*>(d_blob + off[k][1]);
    d.other = reinterpret_cast<const i64*>(d_blob + off[k][2]);
    d.agg = reinterpret_cast<const i64*>(d_blob + off[k][3]);
    d.k = sets[k].n_ranges;
    d.op = sets[k].op;
    d.value = sets[k].out_value;
    d.valid = sets[k].out_valid;
    a4 |= (uintptr_t)d.value | (uintptr_t)d.valid;
  }
  const int vec_ok = (a16 & 15) == 0 && (a4 & 3) == 0;
  const u64 n_tiles = ((u64)n + RSET_TILE - 1) / RSET_TILE;
  // the 28 KB of LDS let five blocks share a compute unit: one resident wave of blocks walks the tiles
  u64 grid = (u64)ctx->n_cu * 5;
  if (grid > n_tiles) grid = n_tiles;
  {
    Phase ph(ctx, st, GIQL_PH_AUX);
    hipLaunchKernelGGL(k_range_set_any, dim3((u32)grid, (u32)n_sets), dim3(RSET_NT), 0, st, chrom, start, end, valid_chrom,
                       valid_start, valid_end, (u64)n, args, vec_ok);
    GIQL_TRY(post_launch("range_set_any"));
  }
  HIP_TRY(hipStreamSynchronize(st));  // (the host block is read by the copy until here)
  collect_spans(ctx);
  ctx->stats.n_out = n;
  return GIQL_OK;
}

// --------------------------------------------------------- LEFT OUTER: the pad
// Mark, count and fill over a flag byte and a bit per left row in the arena (outer_kernels.hip.h); one read-back
// between the count and the fill yields the status and the number of unmatched rows.
int giql_hip_left_pad_dev(giql_hip_ctx* ctx, int32_t* row_a, int32_t* row_b, int64_t n_pairs,
                          int64_t capacity, int64_t n_rows_a, void* stream, int64_t* n_total) {
  if (!ctx || !n_total || n_pairs < 0 || capacity < n_pairs || n_rows_a < 0 || n_rows_a > 0x7FFFFFFFll ||
      (capacity > 0 && !row_a))
    return set_err(GIQL_ERR_INVALID, "bad arguments (0 <= n_pairs <= capacity, n_rows_a < 2^31)");
  *n_total = n_pairs;
  GIQL_TRY(begin_call(ctx));  // (before the way out with nothing to do: that one drops a plan too)
  if (n_pairs == 0 && n_rows_a == 0) return GIQL_OK;
  hipStream_t st = (hipStream_t)stream;
  const size_t n_words = ((size_t)n_rows_a + 63) / 64;
  const u32 nb = cdiv((u64)n_rows_a, LP_BLOCK_ROWS);
  u64 *bits = nullptr, *bsums = nullptr;
  uint8_t* flags = nullptr;
  GIQL_TRY(claim_arena(ctx, st, [&](char* base) {
    Carver c{base};
    flags = c.take<uint8_t>((size_t)n_rows_a + 1);
    bits = c.take<u64>(n_words + 1);
    bsums = c.take<u64>((size_t)nb + 1);
    return c.off;
  }));
  HIP_TRY(hipMemsetAsync(ctx->d_meta, 0, sizeof(DevMeta), st));
  if (n_rows_a) HIP_TRY(hipMemsetAsync(flags, 0, (size_t)n_rows_a, st));
  if (n_pairs > 0) {
    u32 grid = cdiv((u64)n_pairs, LP_NT * 8);
    if (grid > GIQL_STREAM_GRID) grid = GIQL_STREAM_GRID;
    Phase ph(ctx, st, GIQL_PH_AUX);
    hipLaunchKernelGGL(k_left_mark, dim3(grid), dim3(LP_NT), 0, st, (const int*)row_a, (u64)n_pairs, (u32)n_rows_a,
                       flags, ctx->d_meta);
    GIQL_TRY(post_launch("left_mark"));
  }
  if (nb) {
    {
      Phase ph(ctx, st, GIQL_PH_COUNT);
      hipLaunchKernelGGL(k_left_count, dim3(nb), dim3(LP_NT), 0, st, (const uint8_t*)flags, (u32)n_rows_a, bits, bsums);
      GIQL_TRY(post_launch("left_count"));
    }
    Phase ph(ctx, st, GIQL_PH_SCAN);
    hipLaunchKernelGGL(k_scan_spine, dim3(1), dim3(1024), 0, st, bsums, nb, (u64*)nullptr, &ctx->d_meta->n_out);
    GIQL_TRY(post_launch("left_pad scan"));
  }
  const int rc = read_meta(ctx, st);
  if (rc == GIQL_ERR_INVALID)
    return set_err(GIQL_ERR_INVALID, "row_a holds an id outside [0, n_rows_a = %lld)", (long long)n_rows_a);
  GIQL_TRY(rc);
  const u64 n_pad = ctx->h_meta->n_out;
  *n_total = n_pairs + (int64_t)n_pad;
  ctx->stats.n_out = *n_total;
  if (capacity < *n_total) {
    collect_spans(ctx);
    return set_err(GIQL_ERR_CAPACITY, "left_pad: %lld entries offered, %lld needed", (long long)capacity,
                   (long long)*n_total);
  }
  if (n_pad) {
    {
      Phase ph(ctx, st, GIQL_PH_FILL);
      hipLaunchKernelGGL(k_left_fill, dim3(nb), dim3(LP_NT), 0, st, (const u64*)bits, (u32)n_rows_a, (const u64*)bsums,
                         (u64)n_pairs, row_a, row_b);
      GIQL_TRY(post_launch("left_fill"));
    }
    // (the fill stays in flight, like giql_hip_inner_fill_dev's: the total is on the host already)
    if (ctx->profiling) HIP_TRY(hipStreamSynchronize(st));
  }
  collect_spans(ctx);
  return GIQL_OK;
}

// ----------------------------------------------------- host-buffer variants
struct DevSide {
  giql_side s;
  DevArray<int32_t> buf;  // the three columns, uploaded
};

static int upload_side(const giql_side* h, DevSide& d) {
  d.s = *h;
  if (h->n == 0) {
    d.s.chrom = d.s.start = d.s.end = nullptr;
    return GIQL_OK;
  }
  const size_t n = (size_t)h->n;
  GIQL_TRY(d.buf.alloc(3 * n * sizeof(int32_t)));
  HIP_TRY(hipMemcpy(d.buf, h->chrom, n * sizeof(int32_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d.buf + n, h->start, n * sizeof(int32_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d.buf + 2 * n, h->end, n * sizeof(int32_t), hipMemcpyHostToDevice));
  d.s.chrom = d.buf;
  d.s.start = d.buf + n;
  d.s.end = d.buf + 2 * n;
  return GIQL_OK;
}

// the per-row host calls (SEMI / ANTI, COUNT, NEAREST), once their arguments are checked: both sides onto the context's device
static int upload_sides(giql_hip_ctx* ctx, const giql_side* a, const giql_side* b, DevSide& da, DevSide& db) {
  HIP_TRY(hipSetDevice(ctx->device));
  GIQL_TRY(upload_side(a, da));
  return upload_side(b, db);
}

// library-owned host outputs (released by giql_hip_free_host): one process-wide pool (host_pool.h), at most GIQL_HIP_HOST_POOL_MB (default 8192; 0 = none) idle
static void* pinned_alloc(size_t bytes) {
  void* p = nullptr;
  return hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess ? p : nullptr;
}
static void pinned_free(void* p) { (void)hipHostFree(p); }
static HostPool& host_pool() {
  static const char* e = getenv("GIQL_HIP_HOST_POOL_MB");
  // never destroyed: no HIP calls at process exit
  static HostPool* pool = new HostPool((size_t)(e ? strtoull(e, nullptr, 10) : 8192ull) << 20, pinned_alloc, pinned_free);
  return *pool;
}
static void* host_alloc(size_t bytes, bool pinned = true) { return host_pool().get(bytes, pinned); }

int giql_hip_host_pool_trim(int64_t keep_bytes, int64_t* released) {
  if (keep_bytes < 0) return set_err(GIQL_ERR_INVALID, "keep_bytes < 0");
  const size_t freed = host_pool().release_idle((size_t)keep_bytes, true);  // the largest first: they are what a trim is called for
  if (released) *released = (int64_t)freed;
  return GIQL_OK;
}

// ---- the host-buffer INNER join, pipelined over row blocks of the larger table (round 3) ----
// One shot, the call is a chain on the PCIe link: 1.3 GB of columns in (23 ms), the join (2.4 ms), 3.2 GB of
// pairs out (57 ms).  The link is full duplex and an INNER join is a union over row blocks of one side --
// A x B = U_j A x B_j -- so the larger table goes up block by block: while block j's pairs travel to the host on a
// copy stream, block j + 1's columns travel to the device (the host thread sits in that copy) and its join runs;
// only the first upload and the last download stand alone.  The smaller table is uploaded once and sorted again
// per block (a fraction of a millisecond each).  Row ids of the blocked table get the block's first row added on
// the device.  GIQL_HIP_E2E_BLOCK_ROWS: rows per block (default 4M; 0 = one shot).  Measured at 10M x 100M on a
// settled context: 83 ms one shot, 88 / 76 / 71 / 73 ms with blocks of 16M / 8M / 4M / 2M rows -- an upload next to a
// download runs at 25-40 GB/s instead of 56, so the two directions overlap only in part.
__global__ __launch_bounds__(256) void k_add_i32(int32_t* __restrict__ v, u64 n, int32_t add) {
  const u64 stride = (u64)gridDim.x * 256;
  for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) v[i] += add;
}

struct E2eResources {  // released on every path out of inner_host_pipelined
  hipStream_t cs = nullptr;
  hipEvent_t filled[2] = {nullptr, nullptr}, copied[2] = {nullptr, nullptr};
  DevArray<int32_t> in[2];
  DevArray<int32_t> out[2];  // row_a | row_b of a block, half of the buffer each
  HostPtr<int32_t> ha, hb;
  size_t h_cap = 0;
  // the copy stream has drained before the members above, which it reads and writes, are released (after this body)
  ~E2eResources() {
    if (cs) (void)hipStreamSynchronize(cs);
    for (int k = 0; k < 2; k++) {
      if (filled[k]) (void)hipEventDestroy(filled[k]);
      if (copied[k]) (void)hipEventDestroy(copied[k]);
    }
    if (cs) (void)hipStreamDestroy(cs);
  }
};

static int inner_host_pipelined(giql_hip_ctx* ctx, const giql_side* a, const giql_side* b, int32_t n_chrom,
                                size_t block_rows, int64_t* n_pairs, int32_t** row_a, int32_t** row_b) {
  const bool b_big = b->n >= a->n;
  const giql_side* big = b_big ? b : a;
  const giql_side* small = b_big ? a : b;
  DevSide dsmall;
  GIQL_TRY(upload_side(small, dsmall));
  E2eResources R;
  const bool dbg = getenv("GIQL_HIP_DEBUG_E2E") != nullptr;
  HIP_TRY(hipStreamCreateWithFlags(&R.cs, hipStreamNonBlocking));
  for (int k = 0; k < 2; k++) {
    HIP_TRY(hipEventCreateWithFlags(&R.filled[k], hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&R.copied[k], hipEventDisableTiming));
    GIQL_TRY(R.in[k].alloc(3 * block_rows * sizeof(int32_t)));
  }
  const size_t n_big = (size_t)big->n;
  size_t total = 0;
  int slot = 0;
  for (size_t j0 = 0; j0 < n_big; j0 += block_rows, slot ^= 1) {
    const size_t nblk = n_big - j0 < block_rows ? n_big - j0 : block_rows;
    // this slot's columns were last read by the join of two blocks ago, its pairs last copied out then too
    HIP_TRY(hipEventSynchronize(R.filled[slot]));
    int32_t* in = R.in[slot];
    const auto t_up = std::chrono::steady_clock::now();
    // (plain synchronous copies: issued on a stream of their own they took twice as long next to the downloads)
    HIP_TRY(hipMemcpy(in, big->chrom + j0, nblk * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(in + block_rows, big->start + j0, nblk * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(in + 2 * block_rows, big->end + j0, nblk * sizeof(int32_t), hipMemcpyHostToDevice));
    if (dbg)
      fprintf(stderr, "[giql_hip_inner] block at row %zu: upload %.2f ms\n", j0,
              std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_up).count());
    giql_side blk = *big;
    blk.chrom = in;
    blk.start = in + block_rows;
    blk.end = in + 2 * block_rows;
    blk.n = (int64_t)nblk;
    int64_t nj = 0;
    GIQL_TRY(giql_hip_inner_plan_dev(ctx, b_big ? &dsmall.s : &blk, b_big ? &blk : &dsmall.s, n_chrom, nullptr, &nj));
    HIP_TRY(hipEventSynchronize(R.copied[slot]));  // the slot's previous pairs have left the device
    if (nj > 0) {
      const size_t stride = align_up((size_t)nj, (size_t)1 << 19);  // each row on a 2 MiB boundary (the fill's stores)
      {
        const int rc = R.out[slot].grow(2 * stride * sizeof(int32_t), 2 * (stride + stride / 8) * sizeof(int32_t), nullptr, "the pairs");
        if (rc == GIQL_ERR_NOMEM) return set_err(GIQL_ERR_NOMEM, "hipMalloc for %lld pairs failed", (long long)nj);
        GIQL_TRY(rc);
      }
      int32_t* oa = R.out[slot];
      int32_t* ob = oa + R.out[slot].bytes() / (2 * sizeof(int32_t));
      GIQL_TRY(giql_hip_inner_fill_dev(ctx, oa, ob, nj, nullptr));
      if (j0 > 0) {
        u32 grid = cdiv((u64)nj, 256 * 8);
        if (grid > GIQL_STREAM_GRID) grid = GIQL_STREAM_GRID;
        hipLaunchKernelGGL(k_add_i32, dim3(grid), dim3(256), 0, (hipStream_t) nullptr, b_big ? ob : oa, (u64)nj, (int32_t)j0);
        GIQL_TRY(post_launch("row id offset"));
      }
      // host arrays: sized from the first block's yield (the pool usually hands back the previous call's arrays)
      if (total + (size_t)nj > R.h_cap) {
        HIP_TRY(hipStreamSynchronize(R.cs));  // nothing in flight into the arrays that are replaced
        const double per_row = (double)(total + (size_t)nj) / (double)(j0 + nblk);
        size_t want = (size_t)(per_row * (double)n_big * 1.08) + (1u << 20);
        if (want < total + (size_t)nj) want = total + (size_t)nj;
        HostPtr<int32_t> na_(host_alloc(want * sizeof(int32_t))), nb_(host_alloc(want * sizeof(int32_t)));
        if (!na_ || !nb_) return set_err(GIQL_ERR_NOMEM, "out of host memory for %zu pairs", want);
        if (total) {
          memcpy(na_, R.ha, total * sizeof(int32_t));
          memcpy(nb_, R.hb, total * sizeof(int32_t));
        }
        R.ha = std::move(na_);  // (the arrays they replace go back to the pool)
        R.hb = std::move(nb_);
        R.h_cap = want;
      }
      HIP_TRY(hipEventRecord(R.filled[slot], nullptr));
      HIP_TRY(hipStreamWaitEvent(R.cs, R.filled[slot], 0));
      HIP_TRY(hipMemcpyAsync(R.ha + total, oa, (size_t)nj * sizeof(int32_t), hipMemcpyDeviceToHost, R.cs));
      HIP_TRY(hipMemcpyAsync(R.hb + total, ob, (size_t)nj * sizeof(int32_t), hipMemcpyDeviceToHost, R.cs));
      HIP_TRY(hipEventRecord(R.copied[slot], R.cs));
      total += (size_t)nj;
    }
  }
  HIP_TRY(hipStreamSynchronize(R.cs));
  if (!R.ha) {  // no pair at all: the caller still gets arrays to free
    R.ha = HostPtr<int32_t>(host_alloc(sizeof(int32_t)));
    R.hb = HostPtr<int32_t>(host_alloc(sizeof(int32_t)));
    if (!R.ha || !R.hb) return set_err(GIQL_ERR_NOMEM, "out of host memory");
  }
  *n_pairs = (int64_t)total;
  *row_a = R.ha.release();  // handed over
  *row_b = R.hb.release();
  return GIQL_OK;
}

// ---- the host-buffer INNER join with a COMPACT-PLAN download (round 4; GIQL_HIP_E2E_COMPACT=1) ----
// 3.2 GB of pairs take 57 ms on the PCIe link; the plan they are made of -- per query row {row id, first match,
// count} + the other side's row ids in sorted order, giql_hip_inner_plan_export_dev -- is 0.52 GB at the headline
// sizes (9 ms), and host threads expand it at the host's memory rate (tools/probes/host_expand_probe.cpp: 150 GB/s
// of pairs with 16 threads on the GPU box = 21 ms for 3.2 GB).  So: columns up, plan, export, the three per-query
// arrays down, then the sorted ids in chunks while the threads already expand the queries whose ranges have arrived
// (plan_expand.h: blocks of 65,536 queries handed out in order; a block waits for the chunk that holds its furthest id).  The pairs
// come out in the plan's query order.  Only the single-range form (fixed-length side, no irregular rows) has a compact
// plan: any other plan is filled and downloaded as before.  GIQL_HIP_E2E_THREADS: expansion threads (default 32: tools/e2e_threads.py -- 16: 45.8 ms, 32: 39.9, 64: 40.0 at the headline sizes).
static bool plan_has_compact_form(const giql_hip_ctx* ctx) {
  return ctx->plan.inner.uniform != 0 && ctx->plan.n_irr == 0 && ctx->plan.n_c1 == 0 && !ctx->plan.plan_is_join;
}

// returns GIQL_OK with *done = false when the plan has no compact form (the caller fills and downloads)
static int inner_host_compact_tail(giql_hip_ctx* ctx, int64_t n, int32_t* ha, int32_t* hb, bool* done) {
  *done = false;
  if (n <= 0 || !plan_has_compact_form(ctx)) return GIQL_OK;
  const bool q_is_a_plan = ctx->plan.inner.uniform != 2;
  const size_t nq = (size_t)(q_is_a_plan ? ctx->plan.n_a : ctx->plan.n_b), ns = (size_t)(q_is_a_plan ? ctx->plan.n_b : ctx->plan.n_a);
  if (nq == 0 || ns == 0) return GIQL_OK;
  // device staging: the context's output staging buffer (3 nq + ns words)
  const size_t need = (3 * nq + ns + 64) * sizeof(u32);
  GIQL_TRY(ctx->stage_out.grow(need, need + need / 16, nullptr, "the compact plan"));
  int32_t* d_qrid = (int32_t*)ctx->stage_out.get();
  u32* d_lo = (u32*)d_qrid + nq;
  u32* d_cnt = d_lo + nq;
  int32_t* d_srid = (int32_t*)(d_cnt + nq);
  int32_t query_is_a = 0;
  int64_t xq = 0, xs = 0;
  const int rc_x = giql_hip_inner_plan_export_dev(ctx, d_qrid, d_lo, d_cnt, d_srid, (int64_t)nq, (int64_t)ns, 0, 0,
                                                  &query_is_a, &xq, &xs, nullptr);
  if (rc_x == GIQL_ERR_STATE) return GIQL_OK;
  GIQL_TRY(rc_x);
  if ((size_t)xq != nq || (size_t)xs != ns) return set_err(GIQL_ERR_STATE, "plan export sizes changed under the call");
  // page-locked staging of the plan, back to the pool on every path out
  HostPtr<int32_t> h_qrid(host_alloc(nq * 4));
  HostPtr<u32> h_lo(host_alloc(nq * 4)), h_cnt(host_alloc(nq * 4));
  HostPtr<int32_t> h_srid(host_alloc(ns * 4));
  if (!h_qrid || !h_lo || !h_cnt || !h_srid) return set_err(GIQL_ERR_NOMEM, "out of host memory for the compact plan");
  constexpr size_t CHUNK = (size_t)16 << 20;   // sorted ids per download chunk (64 MB: ~1.1 ms on the link)
  constexpr size_t QBLK = (size_t)1 << 16;     // queries per expansion block
  const size_t n_chunks = (ns + CHUNK - 1) / CHUNK;
  std::vector<hipEvent_t> ev(n_chunks + 1, nullptr);
  struct EvGuard {
    std::vector<hipEvent_t>& e;
    ~EvGuard() {
      for (hipEvent_t x : e)
        if (x) (void)hipEventDestroy(x);
    }
  } ev_guard{ev};
  for (auto& e : ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  hipStream_t st = nullptr;  // the export kernel ran on the null stream: the copies follow it there
  HIP_TRY(hipMemcpyAsync(h_cnt, d_cnt, nq * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(h_lo, d_lo, nq * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(h_qrid, d_qrid, nq * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipEventRecord(ev[0], st));
  for (size_t c = 0; c < n_chunks; c++) {
    const size_t c0 = c * CHUNK, cn = ns - c0 < CHUNK ? ns - c0 : CHUNK;
    HIP_TRY(hipMemcpyAsync(h_srid + c0, d_srid + c0, cn * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(ev[c + 1], st));
  }
  HIP_TRY(hipEventSynchronize(ev[0]));  // the per-query arrays are here
  int n_thr = 32;
  if (const char* e = getenv("GIQL_HIP_E2E_THREADS")) n_thr = atoi(e);
  const int hw = (int)std::thread::hardware_concurrency();
  if (hw > 0 && n_thr > hw) n_thr = hw;
  bool stream_stores = true;  // GIQL_HIP_E2E_NT=0: plain stores
  if (const char* e = getenv("GIQL_HIP_E2E_NT")) stream_stores = atoi(e) != 0;
  // (both output arrays come page-aligned from the pool: expand_plan's precondition)
  GIQL_TRY(expand_plan(CompactPlan{h_qrid, h_lo, h_cnt, h_srid, nq, ns}, (uint64_t)n, query_is_a ? ha : hb, query_is_a ? hb : ha,
                       n_thr, stream_stores, CHUNK, QBLK, [&](size_t c) { return hipEventSynchronize(ev[c + 1]) != hipSuccess; }, set_err));
  *done = true;
  return GIQL_OK;
}

int giql_hip_inner(giql_hip_ctx* ctx, const giql_side* a, const giql_side* b, int32_t n_chrom,
                   int64_t* n_pairs, int32_t** row_a, int32_t** row_b) {
  if (!ctx || !n_pairs || !row_a || !row_b) return set_err(GIQL_ERR_INVALID, "NULL argument");
  GIQL_TRY(check_side(a, "a"));
  GIQL_TRY(check_side(b, "b"));
  HIP_TRY(hipSetDevice(ctx->device));
  *row_a = *row_b = nullptr;
  // The plans made below read sides staged on the device for this call only: none outlives it.  (The one write of
  // the tag outside the plan entry points, begin_call and the arena: a plan must not point at released columns.)
  struct DropPlan {
    giql_hip_ctx* c;
    ~DropPlan() { c->kept = Plan::NONE; }
  } drop_plan{ctx};
  // GIQL_HIP_E2E_COMPACT: 1 = compact-plan download whenever the plan has that form, 0 = never (round 3: pairs
  // downloaded, the larger table uploaded block by block); unset = compact unless this context's last plan says the
  // tables do not take the single-range form (then the block pipeline, which hides most of the upload, is the better bet)
  const char* e_compact = getenv("GIQL_HIP_E2E_COMPACT");
  const int compact_mode = e_compact ? (atoi(e_compact) != 0 ? 1 : 0) : -1;
  const bool try_compact = compact_mode == 1 ||
                           (compact_mode < 0 && !(ctx->guess.spec_valid && (ctx->guess.spec_form == 0 || !ctx->guess.last_no_irr)));
  if (!try_compact) {
    const char* e = getenv("GIQL_HIP_E2E_BLOCK_ROWS");
    const size_t block_rows = e ? (size_t)strtoull(e, nullptr, 10) : ((size_t)4 << 20);
    const size_t n_big = (size_t)(a->n > b->n ? a->n : b->n);
    if (block_rows > 0 && n_big >= 2 * block_rows && a->n > 0 && b->n > 0)
      return inner_host_pipelined(ctx, a, b, n_chrom, block_rows, n_pairs, row_a, row_b);
  }
  // GIQL_HIP_DEBUG_E2E=1: where the PCIe-inclusive call spends its wall time (stderr)
  const bool dbg = getenv("GIQL_HIP_DEBUG_E2E") != nullptr;
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms_since = [&](std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(now() - t).count();
  };
  auto t0 = now();
  DevSide da, db;
  GIQL_TRY(upload_side(a, da));
  GIQL_TRY(upload_side(b, db));
  const double ms_h2d = ms_since(t0);
  t0 = now();
  int64_t n = 0;
  GIQL_TRY(giql_hip_inner_plan_dev(ctx, &da.s, &db.s, n_chrom, nullptr, &n));
  const double ms_plan = ms_since(t0);
  t0 = now();
  *n_pairs = n;
  // The compact plan pays when it is smaller than the pairs (and the result is worth a team of threads)
  bool compact = false;
  if (try_compact && n > 0 && plan_has_compact_form(ctx)) {
    const bool q_is_a_plan = ctx->plan.inner.uniform != 2;
    const int64_t nq = q_is_a_plan ? ctx->plan.n_a : ctx->plan.n_b, ns = q_is_a_plan ? ctx->plan.n_b : ctx->plan.n_a;
    // ... on a host with the cores to expand it: 16 threads write ~150 GB/s of pairs, 4 would lose against the link
    const unsigned hw = std::thread::hardware_concurrency();
    compact = compact_mode == 1 || (n >= (4ll << 20) && 8 * n >= 12 * nq + 4 * ns && hw >= 16);
  }
  // library-owned host outputs are PINNED (the D2H copy of the pairs runs at link speed, not through a pageable
  // bounce buffer) -- unless host threads write them (compact plan): plain memory then, nothing to page-lock (3.2 GB:
  // ~200 ms on a first call); giql_hip_free_host releases either kind
  const size_t out_bytes = (size_t)(n > 0 ? n : 1) * sizeof(int32_t);
  HostPtr<int32_t> ha(host_alloc(out_bytes, !compact));
  HostPtr<int32_t> hb(host_alloc(out_bytes, !compact));
  if (!ha || !hb) return set_err(GIQL_ERR_NOMEM, "out of host memory for %lld pairs", (long long)n);
  const double ms_pin = ms_since(t0);
  t0 = now();
  double ms_fill = 0, ms_d2h = 0;
  bool compact_done = false;
  if (compact && n > 0) GIQL_TRY(inner_host_compact_tail(ctx, n, ha, hb, &compact_done));
  if (n > 0 && !compact_done) {
    // row_b starts on a 2 MiB boundary of its own: a row that begins in the middle of a cache
    // line makes every 256-byte wave store of the fill touch three lines instead of two
    const size_t stride = align_up((size_t)n, (size_t)1 << 19);
    // the device staging of the pairs is kept by the context (a fresh 3.2 GB hipMalloc costs ~160 ms)
    const size_t need = 2 * stride * sizeof(int32_t);
    int rc = ctx->stage_out.grow(need, need + need / 16, nullptr, "the pairs");
    int32_t* d_a = (int32_t*)ctx->stage_out.get();
    int32_t* d_b = d_a + stride;
    if (rc == GIQL_OK) rc = giql_hip_inner_fill_dev(ctx, d_a, d_b, n, nullptr);
    if (dbg) {
      (void)hipDeviceSynchronize();
      ms_fill = ms_since(t0);
      t0 = now();
    }
    if (rc == GIQL_OK && hipMemcpy(ha, d_a, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess)
      rc = set_err(GIQL_ERR_HIP, "D2H copy of row_a failed");
    if (rc == GIQL_OK && hipMemcpy(hb, d_b, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess)
      rc = set_err(GIQL_ERR_HIP, "D2H copy of row_b failed");
    GIQL_TRY(rc);
  }
  ms_d2h = ms_since(t0);
  if (dbg)
    fprintf(stderr, "[giql_hip_inner] H2D %.1f ms, plan %.1f, pinned alloc %.1f, output alloc + fill %.1f, %s %.1f (%lld pairs)\n",
            ms_h2d, ms_plan, ms_pin, ms_fill, compact_done ? "compact plan D2H + host expansion" : "D2H", ms_d2h, (long long)n);
  *row_a = ha.release();
  *row_b = hb.release();
  return GIQL_OK;
}

int giql_hip_semi_anti(giql_hip_ctx* ctx, const giql_side* a, const giql_side* b, int32_t n_chrom,
                       int anti, int64_t* n_out, int32_t** rows_a) {
  if (!ctx || !n_out || !rows_a) return set_err(GIQL_ERR_INVALID, "NULL argument");
  GIQL_TRY(check_side(a, "a"));
  GIQL_TRY(check_side(b, "b"));
  *rows_a = nullptr;
  DevSide da, db;
  GIQL_TRY(upload_sides(ctx, a, b, da, db));
  DevArray<int32_t> out;
  const size_t na = (size_t)a->n;
  GIQL_TRY(out.alloc((na ? na : 1) * sizeof(int32_t)));
  int64_t n = 0;
  GIQL_TRY(giql_hip_semi_anti_dev(ctx, &da.s, &db.s, n_chrom, anti, out, &n, nullptr));
  HostPtr<int32_t> h(host_alloc((size_t)(n > 0 ? n : 1) * sizeof(int32_t)));
  if (!h) return set_err(GIQL_ERR_NOMEM, "out of host memory");
  if (n > 0 && hipMemcpy(h, out, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess)
    return set_err(GIQL_ERR_HIP, "D2H copy failed");
  *n_out = n;
  *rows_a = h.release();
  return GIQL_OK;
}

int giql_hip_count(giql_hip_ctx* ctx, const giql_side* a, const giql_side* b, int32_t n_chrom,
                   int64_t* counts_out) {
  if (!ctx) return set_err(GIQL_ERR_INVALID, "NULL argument");
  GIQL_TRY(check_side(a, "a"));
  GIQL_TRY(check_side(b, "b"));
  if (a->n == 0) return GIQL_OK;
  if (!counts_out) return set_err(GIQL_ERR_INVALID, "counts_out is NULL");
  DevSide da, db;
  GIQL_TRY(upload_sides(ctx, a, b, da, db));
  DevArray<int64_t> out;
  GIQL_TRY(out.alloc((size_t)a->n * sizeof(int64_t)));
  GIQL_TRY(giql_hip_count_dev(ctx, &da.s, &db.s, n_chrom, out, nullptr));
  HIP_TRY(hipMemcpy(counts_out, out, (size_t)a->n * sizeof(int64_t), hipMemcpyDeviceToHost));
  return GIQL_OK;
}

int giql_hip_nearest(giql_hip_ctx* ctx, const giql_side* a, const giql_side* b, int32_t n_chrom,
                     int is_signed, int64_t max_distance, int32_t* idx_b_out, int64_t* dist_out) {
  if (!ctx) return set_err(GIQL_ERR_INVALID, "NULL argument");
  GIQL_TRY(check_side(a, "a"));
  GIQL_TRY(check_side(b, "b"));
  if (a->n == 0) return GIQL_OK;
  if (!idx_b_out || !dist_out) return set_err(GIQL_ERR_INVALID, "output is NULL");
  DevSide da, db;
  GIQL_TRY(upload_sides(ctx, a, b, da, db));
  DevArray<int32_t> oi;
  DevArray<int64_t> od;
  GIQL_TRY(oi.alloc((size_t)a->n * sizeof(int32_t)));
  GIQL_TRY(od.alloc((size_t)a->n * sizeof(int64_t)));
  GIQL_TRY(giql_hip_nearest_dev(ctx, &da.s, &db.s, n_chrom, is_signed, max_distance, oi, od, nullptr));
  HIP_TRY(hipMemcpy(idx_b_out, oi, (size_t)a->n * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(dist_out, od, (size_t)a->n * sizeof(int64_t), hipMemcpyDeviceToHost));
  return GIQL_OK;
}

void giql_hip_free_host(void* p) {
  if (p) host_pool().put(p);
}

#if defined(GIQL_OS_TIMELINE)
// diagnostic builds only (tools/os_timeline.py): the phase stamps of the last sort pass
int giql_hip_debug_timeline(unsigned long long* out, int64_t n_words) {
  const size_t cap = (size_t)OS_TL_TILES * 16;
  const size_t n = (size_t)n_words < cap ? (size_t)n_words : cap;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_os_tl), n * sizeof(unsigned long long)));
  return GIQL_OK;
}
#endif

}  // extern "C"
