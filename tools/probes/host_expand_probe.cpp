// Host-side expansion of a compact join plan (VERDICT r03 "Next round" 8: would a compact-plan download + expansion by
// host threads beat moving the 3.2 GB of pairs over PCIe?).  Synthetic plan of the headline's shape: 10M query rows,
// ~40 pairs each, a 100M-entry sorted-id array, expanded by the library's own expander (giql_amd/csrc/plan_expand.h,
// its chunk and block sizes, every chunk already there) into arrays that have been touched before (as the library's
// pool hands them out).  Prints GB/s of pairs written per thread count, for plain and for non-temporal stores.
//   g++ -O3 -march=native -pthread -o /tmp/host_expand_probe tools/probes/host_expand_probe.cpp && /tmp/host_expand_probe
#include <chrono>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../../giql_amd/csrc/plan_expand.h"

static int report(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  return code;
}

int main() {
  const size_t nq = 10000000, ns = 100000000;
  std::vector<uint32_t> lo(nq), cnt(nq);
  std::vector<int32_t> qrid(nq), srid(ns);
  uint64_t x = 88172645463325252ull;
  auto rnd = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  for (size_t i = 0; i < ns; i++) srid[i] = (int32_t)(rnd() % ns);
  uint64_t total = 0;
  for (size_t i = 0; i < nq; i++) {
    cnt[i] = 20 + (uint32_t)(rnd() % 41);
    lo[i] = (uint32_t)((i * 10ull + rnd() % 8) % (ns - 64));
    qrid[i] = (int32_t)(rnd() % nq);
    total += cnt[i];
  }
  const size_t bytes = (total * 4 + 4095) / 4096 * 4096;
  int32_t* ra = (int32_t*)aligned_alloc(4096, bytes);
  int32_t* rb = (int32_t*)aligned_alloc(4096, bytes);
  memset(ra, 0, bytes);
  memset(rb, 0, bytes);
  const unsigned hw = std::thread::hardware_concurrency();
  printf("pairs %llu (%.2f GB of output), hardware_concurrency %u\n", (unsigned long long)total, total * 8 / 1e9, hw);
  for (const bool stream : {false, true})
    for (int T : {8, 16, 32, 64, 128}) {
      if ((unsigned)T > hw) break;
      double best = 1e30;
      for (int rep = 0; rep < 3; rep++) {
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = expand_plan(CompactPlan{qrid.data(), lo.data(), cnt.data(), srid.data(), nq, ns}, total, ra, rb, T, stream,
                                   (size_t)16 << 20, (size_t)1 << 16, [](size_t) { return 0; }, report);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (rc != GIQL_OK) return 1;
        if (ms < best) best = ms;
      }
      printf("%s stores, threads %3d: %.1f ms = %.1f GB/s of pairs written\n", stream ? "non-temporal" : "plain       ", T, best,
             total * 8 / 1e6 / best);
    }
  return 0;
}
