// tests/native/host_side_check.cpp -- the pure-host half of giql_hip_inner, checked without a GPU: the expansion of a
// compact plan by a team of threads (plan_expand.h) against a serial reference, and the host pool's policy
// (host_pool.h) over a counting fake of the page-locked allocator.  One line per case; exits non-zero on the first
// failure.  Drivers: tests/test_host_side_cpu.py (plain build), tools/host_side_sanitize.sh (ASan + UBSan, TSan).
//   g++ -std=c++17 -pthread -o host_side_check tests/native/host_side_check.cpp && ./host_side_check
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <thread>
#include <vector>

#include "../../giql_amd/csrc/host_pool.h"
#include "../../giql_amd/csrc/plan_expand.h"

#define CHECK(cond, ...)                                      \
  do {                                                        \
    if (!(cond)) {                                            \
      printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
      printf(__VA_ARGS__);                                    \
      printf("\n");                                           \
      exit(1);                                                \
    }                                                         \
  } while (0)

// ------------------------------------------------------------------------------------------------- the expansion
constexpr size_t CHUNK = 64;  // ids per chunk
constexpr size_t QBLK = 8;    // queries per block
constexpr size_t GUARD = 16;  // entries before and after each output (one 64-byte line: the outputs stay aligned)
constexpr int32_t UNTOUCHED = 0x5A5A5A5A, NOT_HERE_YET = -7;

struct Plan {
  std::vector<int32_t> q_rid;
  std::vector<uint32_t> lo, cnt;
  std::vector<int32_t> s_rid;
  uint64_t pairs() const {
    uint64_t t = 0;
    for (uint32_t c : cnt) t += c;
    return t;
  }
};

// nq queries with the given counts; each range starts wherever `lo_of(q)` says
static Plan make_plan(const std::vector<uint32_t>& cnt, size_t ns, const std::function<uint32_t(size_t)>& lo_of) {
  Plan p;
  p.cnt = cnt;
  for (size_t q = 0; q < cnt.size(); q++) {
    p.q_rid.push_back((int32_t)(1000 + 7 * q));
    p.lo.push_back(lo_of(q));
  }
  for (size_t i = 0; i < ns; i++) p.s_rid.push_back((int32_t)(i * 2654435761u % 100003));
  return p;
}
// ranges spread over the sorted ids, each one inside them
static Plan make_plan(const std::vector<uint32_t>& cnt, size_t ns) {
  return make_plan(cnt, ns, [&](size_t q) { return cnt[q] >= ns ? 0u : (uint32_t)((q * 37) % (ns - cnt[q] + 1)); });
}

static void reference(const Plan& p, std::vector<int32_t>& out_q, std::vector<int32_t>& out_s) {
  for (size_t q = 0; q < p.cnt.size(); q++)
    for (uint32_t k = 0; k < p.cnt[q]; k++) {
      out_q.push_back(p.q_rid[q]);
      out_s.push_back(p.s_rid[p.lo[q] + k]);
    }
}

struct Out {  // a 64-byte aligned output array between two guard lines
  int32_t* base;
  size_t n;
  explicit Out(size_t n_) : n(n_) {
    const size_t bytes = ((n + 2 * GUARD) * sizeof(int32_t) + 63) / 64 * 64;
    base = (int32_t*)aligned_alloc(64, bytes);
    std::fill(base, base + n + 2 * GUARD, UNTOUCHED);
  }
  ~Out() { free(base); }
  int32_t* data() const { return base + GUARD; }
  bool guards_intact() const {
    for (size_t i = 0; i < GUARD; i++)
      if (base[i] != UNTOUCHED || base[GUARD + n + i] != UNTOUCHED) return false;
    return true;
  }
  bool untouched() const { return std::all_of(base, base + n + 2 * GUARD, [](int32_t v) { return v == UNTOUCHED; }); }
};

enum class Arrival { AT_ONCE, ONE_BY_ONE, SECOND_FAILS };

struct Expect {
  int rc = GIQL_OK;
  const char* msg = "";  // a part of the message
};

static char g_msg[256];  // what the library keeps through set_err
static int record_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
  va_end(ap);
  return code;
}

// one case: plain and non-temporal stores, 1, 3 and more-than-blocks threads
static void expansion_case(const char* name, const Plan& p, uint64_t promised, Arrival arrival = Arrival::AT_ONCE,
                           Expect want = Expect(), size_t chunk = CHUNK, size_t qblk = QBLK) {
  const size_t nq = p.cnt.size(), ns = p.s_rid.size(), n_blk = (nq + qblk - 1) / qblk;
  CHECK(n_blk + 1 <= 8, "%s: at most 8 threads", name);
  std::vector<int32_t> ref_q, ref_s;
  if (want.rc == GIQL_OK) reference(p, ref_q, ref_s);
  for (const bool stream : {false, true})
    for (const int n_thr : {1, 3, (int)n_blk + 1}) {
      Out oq(promised), os(promised);
      // the sorted ids the expansion reads: all there, or handed over chunk by chunk by the wait
      std::vector<int32_t> ids(p.s_rid);
      if (arrival != Arrival::AT_ONCE) std::fill(ids.begin(), ids.end(), NOT_HERE_YET);
      size_t waits = 0;
      auto wait_chunk = [&](size_t c) {
        waits++;
        if (arrival == Arrival::AT_ONCE) return 0;
        std::this_thread::sleep_for(std::chrono::milliseconds(1));  // (helpers are waiting for this chunk by now)
        if (arrival == Arrival::SECOND_FAILS && c == 1) return 1;
        const size_t c0 = c * chunk, c1 = std::min(ns, c0 + chunk);
        std::copy(p.s_rid.begin() + (long)c0, p.s_rid.begin() + (long)c1, ids.begin() + (long)c0);
        return 0;
      };
      g_msg[0] = 0;
      const int rc = expand_plan(CompactPlan{p.q_rid.data(), p.lo.data(), p.cnt.data(), ids.data(), nq, ns}, promised,
                                 oq.data(), os.data(), n_thr, stream, chunk, qblk, wait_chunk, record_error);
      const char* msg = g_msg;
      const char* how = stream ? "non-temporal" : "plain";
      CHECK(rc == want.rc, "%s (%s, %d threads): rc %d, message '%s'", name, how, n_thr, rc, msg);
      CHECK(strstr(msg, want.msg) != nullptr, "%s (%s, %d threads): message '%s'", name, how, n_thr, msg);
      CHECK(oq.guards_intact() && os.guards_intact(), "%s (%s, %d threads): wrote outside the outputs", name, how, n_thr);
      if (want.rc == GIQL_OK) {
        CHECK(waits == (ns + chunk - 1) / chunk, "%s: %zu waits", name, waits);
        for (size_t i = 0; i < promised; i++)
          CHECK(oq.data()[i] == ref_q[i] && os.data()[i] == ref_s[i], "%s (%s, %d threads): pair %zu is (%d, %d), want (%d, %d)",
                name, how, n_thr, i, oq.data()[i], os.data()[i], ref_q[i], ref_s[i]);
      } else if (want.rc == GIQL_ERR_STATE) {
        CHECK(waits == 0 && oq.untouched() && os.untouched(), "%s (%s, %d threads): wrote before the error", name, how, n_thr);
      } else {  // the failed wait: every helper has been joined, so nothing is written any more
        CHECK(waits == 2, "%s: %zu waits", name, waits);
        std::vector<int32_t> then_q(oq.data(), oq.data() + promised), then_s(os.data(), os.data() + promised);
        std::this_thread::sleep_for(std::chrono::milliseconds(3));
        CHECK(std::equal(then_q.begin(), then_q.end(), oq.data()) && std::equal(then_s.begin(), then_s.end(), os.data()),
              "%s (%s, %d threads): a thread still writes after the call returned", name, how, n_thr);
      }
    }
  printf("ok   expand: %s\n", name);
}

static void expansion_cases() {
  {
    const Plan p = make_plan(std::vector<uint32_t>(20, 0), 100);
    expansion_case("every count zero", p, 0);
  }
  {
    const Plan p = make_plan({1}, 10);
    expansion_case("one query, one pair", p, 1);
  }
  {  // block 0 leaves 5 pairs: block 1 (9 pairs) lies inside a line, block 2 (7 pairs, from 14) crosses into the next
    const Plan p = make_plan({1, 0, 2, 0, 0, 1, 1, 0, /**/ 3, 0, 0, 4, 0, 1, 1, 0, /**/ 2, 2, 0, 0, 3, 0, 0, 0}, 200);
    expansion_case("short block off a 64-byte line", p, p.pairs());
  }
  for (const uint32_t extra : {0u, 15u}) {  // block 1 starts at pair 5: an aligned head of 11, then one staging buffer exactly
    const Plan p = make_plan({5, 0, 0, 0, 0, 0, 0, 0, /**/ 200, 100, 300, 35, 0, 150, 250 + extra, 0}, 512);
    CHECK(p.pairs() == 5 + 11 + 1024 + extra, "the case's own arithmetic");
    expansion_case(extra ? "block of 1024 + 15 pairs after the head" : "block of 1024 pairs after the head", p, p.pairs());
  }
  {
    const Plan p = make_plan({3, 5000, 2}, 5010);
    expansion_case("one run of 5000 ids across staging refills", p, p.pairs());
  }
  {  // zeros at the end of a block (q 1..7), a whole block of zeros (q 16..23), zeros at the end of the plan (q 41..47)
    std::vector<uint32_t> cnt(48, 0);
    cnt[0] = 3, cnt[8] = 40, cnt[15] = 1, cnt[24] = 1100, cnt[31] = 17, cnt[32] = 2, cnt[40] = 9;
    const Plan p = make_plan(cnt, 1200);
    expansion_case("long stretches of zero counts", p, p.pairs());
  }
  {  // the block's FIRST query reads the last chunk, its last query the first: it must wait for chunk 3, not chunk 0
    const std::vector<uint32_t> cnt = {10, 0, 20, 5, 0, 0, 3, 6};
    const uint32_t lo[] = {240, 0, 100, 70, 0, 0, 130, 2};
    const Plan p = make_plan(cnt, 256, [&](size_t q) { return lo[q]; });
    expansion_case("lo not monotone within a block", p, p.pairs(), Arrival::ONE_BY_ONE);
  }
  {
    const Plan p = make_plan({4, 4, 4, 10, 4}, 100, [](size_t q) { return q == 3 ? 91u : (uint32_t)(q * 5); });
    expansion_case("a range past the sorted ids", p, p.pairs(), Arrival::AT_ONCE, {GIQL_ERR_STATE, "a range past the sorted ids"});
  }
  {
    const Plan p = make_plan({4, 4, 4, 10, 4}, 100);
    expansion_case("counts that miss the promised total", p, p.pairs() + 1, Arrival::AT_ONCE, {GIQL_ERR_STATE, "26 pairs, the plan counted 27"});
  }
  {  // 48 queries = 6 blocks over 4 chunks: block b's ranges end in chunk (b * 4) / 6 or the one after
    std::vector<uint32_t> cnt(48);
    for (size_t q = 0; q < 48; q++) cnt[q] = (uint32_t)(q % 5 == 4 ? 0 : 3 + q % 11);
    const Plan p = make_plan(cnt, 256, [&](size_t q) { return (uint32_t)(q * 5); });
    expansion_case("chunks arrive one at a time", p, p.pairs(), Arrival::ONE_BY_ONE);
    expansion_case("the second of four chunks fails", p, p.pairs(), Arrival::SECOND_FAILS, {GIQL_ERR_HIP, "D2H copy of the compact plan failed"});
  }
}

// ------------------------------------------------------------------------------------------------------ the pool
// the counting fake of the page-locked allocator
static std::mutex g_mu;
static std::map<void*, size_t> g_live;
static size_t g_allocs = 0, g_frees = 0, g_bytes_freed = 0, g_last_request = 0;
static std::vector<void*> g_freed;
static bool g_fail = false;

static void* fake_alloc(size_t bytes) {
  std::lock_guard<std::mutex> g(g_mu);
  g_last_request = bytes;
  if (g_fail) return nullptr;
  void* p = aligned_alloc(4096, (bytes + 4095) / 4096 * 4096);
  g_live[p] = bytes;
  g_allocs++;
  return p;
}
static void fake_free(void* p) {
  std::lock_guard<std::mutex> g(g_mu);
  const auto it = g_live.find(p);
  CHECK(it != g_live.end(), "the pool released %p, which the fake never handed out (or released already)", p);
  g_bytes_freed += it->second;
  g_live.erase(it);
  g_freed.push_back(p);
  g_frees++;
  free(p);
}
static bool was_freed(void* p) { return std::find(g_freed.begin(), g_freed.end(), p) != g_freed.end(); }
static void pool_case_done(HostPool& pool, const char* name) {
  (void)pool.release_idle(0, true);
  CHECK(g_live.empty() && g_allocs == g_frees, "%s: %zu allocations, %zu releases", name, g_allocs, g_frees);
  g_freed.clear();
  g_allocs = g_frees = g_bytes_freed = 0;
  printf("ok   pool: %s\n", name);
}

constexpr size_t MiB = (size_t)1 << 20, NO_LIMIT = (size_t)1 << 40;

static void pool_cases() {
  {
    HostPool pool(NO_LIMIT, fake_alloc, fake_free);
    void* p = pool.get(1000);
    pool.put(p);
    void* q = pool.get(900);
    CHECK(p && q == p && g_allocs == 1, "%p then %p", p, q);
    pool.put(q);
    pool_case_done(pool, "get, put, get of a similar size: the same pointer");
  }
  {
    HostPool pool(NO_LIMIT, fake_alloc, fake_free);
    char* a = (char*)pool.get(1000);
    char* b = (char*)pool.get(1000);
    char* c = (char*)pool.get(1000, false);
    CHECK(a && b && c && (a + 1000 <= b || b + 1000 <= a) && (a + 1000 <= c || c + 1000 <= a) && (b + 1000 <= c || c + 1000 <= b),
          "%p %p %p", (void*)a, (void*)b, (void*)c);
    pool.put(a), pool.put(b), pool.put(c);
    pool_case_done(pool, "two live buffers never alias");
  }
  {
    HostPool pool(NO_LIMIT, fake_alloc, fake_free);
    void *p4 = pool.get(4 * MiB), *p1 = pool.get(1 * MiB), *p2 = pool.get(2 * MiB);
    pool.put(p4), pool.put(p1), pool.put(p2);
    void* q = pool.get(MiB + MiB / 2);
    CHECK(q == p2 && g_allocs == 3, "best fit for 1.5 MiB took %s", q == p4 ? "the 4 MiB buffer" : q == p1 ? "the 1 MiB buffer" : "a new one");
    pool.put(q);
    pool_case_done(pool, "best fit: the smallest sufficient idle buffer");
  }
  {
    HostPool pool(NO_LIMIT, fake_alloc, fake_free);
    void* big = pool.get(8 * MiB);
    pool.put(big);
    void* small = pool.get(4);
    CHECK(small && small != big && g_allocs == 2, "a 4-byte request took the 8 MiB buffer");
    void* again = pool.get(8 * MiB);
    CHECK(again == big, "the 8 MiB buffer is still there for a request of its size");
    pool.put(small), pool.put(again);
    pool_case_done(pool, "a 4-byte request leaves an 8 MiB idle buffer alone");
  }
  {
    HostPool pool(NO_LIMIT, fake_alloc, fake_free);
    void* pinned = pool.get(1000);
    pool.put(pinned);
    void* q = pool.get(1000, false);
    CHECK(q == pinned, "a plain request did not take the idle page-locked buffer");
    pool.put(q);
    void* plain = pool.get(3 * MiB, false);
    CHECK(plain && g_allocs == 1 && (uintptr_t)plain % (2 * MiB) == 0, "a plain buffer: not from the page-locked allocator, on a 2 MiB boundary");
    pool.put(plain);
    void* r = pool.get(3 * MiB);
    CHECK(r && r != plain && g_allocs == 2, "a page-locked request took an idle plain buffer");
    pool.put(r);
    pool_case_done(pool, "page-locked serves plain, plain never serves page-locked");
  }
  {
    HostPool pool(NO_LIMIT, fake_alloc, fake_free);
    void* stranger = fake_alloc(64);
    const size_t before = g_frees;
    pool.put(stranger);
    CHECK(g_frees == before + 1 && was_freed(stranger), "%zu releases", g_frees - before);
    pool_case_done(pool, "put of an unknown pointer: one page-locked release");
  }
  {  // idle buffers of 1, 2 and 4 MiB + 1/16 each = 7.4375 MiB against a limit of 4.5: the 1 and the 2 go, in that order
    HostPool pool(4 * MiB + MiB / 2, fake_alloc, fake_free);
    void *p1 = pool.get(1 * MiB), *p2 = pool.get(2 * MiB), *p4 = pool.get(4 * MiB);
    pool.put(p2), pool.put(p1);
    CHECK(g_frees == 0, "released below the limit");
    pool.put(p4);
    CHECK(g_freed.size() == 2 && g_freed[0] == p1 && g_freed[1] == p2, "%zu releases, the smallest first", g_freed.size());
    void* q = pool.get(4 * MiB);
    CHECK(q == p4, "the largest buffer was not kept");
    pool.put(q);
    pool_case_done(pool, "over the idle limit the smallest go first");
  }
  {
    HostPool pool(0, fake_alloc, fake_free);
    void* p = pool.get(1000);
    pool.put(p);
    CHECK(g_frees == 1 && was_freed(p), "limit 0 kept a buffer");
    void* plain = pool.get(1000, false);
    pool.put(plain);
    void* q = pool.get(1000);
    CHECK(q && g_allocs == 2, "limit 0 kept a buffer");
    pool.put(q);
    pool_case_done(pool, "idle limit 0 keeps nothing");
  }
  {  // 7.4375 MiB idle, trimmed to 3.25: the 4 MiB buffer alone goes
    HostPool pool(NO_LIMIT, fake_alloc, fake_free);
    void *p1 = pool.get(1 * MiB), *p4 = pool.get(4 * MiB), *p2 = pool.get(2 * MiB);
    pool.put(p1), pool.put(p4), pool.put(p2);
    const size_t released = pool.release_idle(3 * MiB + MiB / 4, true);
    CHECK(g_freed.size() == 1 && g_freed[0] == p4, "%zu releases, the largest first", g_freed.size());
    CHECK(released == 4 * MiB + MiB / 4 && released == g_bytes_freed, "trim reports %zu bytes, the fake saw %zu", released, g_bytes_freed);
    void* live = pool.get(2 * MiB);  // a buffer in use is not the trim's to release
    CHECK(live == p2 && pool.release_idle(0, true) == MiB + MiB / 16 && !was_freed(p2), "trim to 0 with a live buffer");
    pool.put(live);
    pool_case_done(pool, "trim to keep_bytes: the largest first, bytes reported");
  }
  {
    HostPool pool(NO_LIMIT, fake_alloc, fake_free);
    void* z = pool.get(0);
    CHECK(z && g_last_request == 1, "a zero-byte request asked the allocator for %zu bytes", g_last_request);
    pool.put(z);
    g_fail = true;
    CHECK(pool.get(64 * MiB) == nullptr, "a failed allocation returned a pointer");
    g_fail = false;
    pool_case_done(pool, "zero bytes served as one; allocation failure returns nullptr");
  }
  {
    std::vector<void*> mine;
    HostPool pool(NO_LIMIT, fake_alloc, fake_free);
    for (size_t b : {100u, 70000u, 3000000u}) mine.push_back(pool.get(b, b != 70000u));
    for (void* p : mine) pool.put(p);
    CHECK(pool.release_idle(0, false) > 0 && g_live.empty() && g_allocs == g_frees, "%zu allocations, %zu releases", g_allocs, g_frees);
    pool_case_done(pool, "everything back and trimmed to 0: allocations and releases balance");
  }
  {  // (for ThreadSanitizer) four threads on one pool with a limit small enough that puts evict
    HostPool pool(MiB, fake_alloc, fake_free);
    std::atomic<int> clashes{0};
    std::vector<std::thread> th;
    for (int t = 0; t < 4; t++)
      th.emplace_back([&, t] {
        uint32_t x = 12345u + (uint32_t)t;
        for (int round = 0; round < 3000; round++) {
          x = x * 1664525u + 1013904223u;
          const size_t bytes = 8 + (x >> 8) % 300000;
          int* p = (int*)pool.get(bytes, (x & 3u) != 0);  // one in four: plain memory
          if (!p) {
            clashes++;
            continue;
          }
          p[0] = t, p[1] = round;
          std::this_thread::yield();
          if (p[0] != t || p[1] != round) clashes++;  // somebody else holds the same buffer
          pool.put(p);
        }
      });
    for (auto& t : th) t.join();
    CHECK(clashes == 0, "%d buffers were shared or missing", clashes.load());
    pool_case_done(pool, "four threads get and put");
  }
}

int main() {
  expansion_cases();
  pool_cases();
  printf("all cases passed\n");
  return 0;
}
