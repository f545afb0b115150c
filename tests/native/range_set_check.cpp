// tests/native/range_set_check.cpp -- giql_amd/csrc/range_set_prepare.h without a GPU: every prepared table is checked
// for its order and its running aggregate, and the one-search lookup over it against the plain OR over the ranges,
// on probe rows placed at, one below and one above every bound.  Stand-alone: builds with any C++17 compiler, with or
// without -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../../giql_amd/csrc/range_set_prepare.h"

using namespace giql;

static int g_failed = 0;

struct Range {
  int32_t chrom;
  int64_t on_start, on_end;
};

static bool term(int op, const Range& r, int32_t c, int64_t s, int64_t e) {
  if (r.chrom != c) return false;
  if (op == RSET_INTERSECTS) return s < r.on_start && e > r.on_end;
  if (op == RSET_CONTAINS) return s <= r.on_start && e >= r.on_end;
  return s >= r.on_start && e <= r.on_end;
}

static void check(const std::string& name, const std::vector<Range>& ranges, const std::vector<int32_t>& probe_chroms,
                  const std::vector<int64_t>& extra = {}) {
  bool ok = true;
  std::vector<int32_t> chrom;
  std::vector<int64_t> bs, be;
  for (const Range& r : ranges) {
    chrom.push_back(r.chrom);
    bs.push_back(r.on_start);
    be.push_back(r.on_end);
  }
  // probe coordinates: every bound, its neighbours (where they exist), and the ends of int32 (what a column can hold)
  std::vector<int64_t> pts = extra;
  for (const Range& r : ranges)
    for (int64_t v : {r.on_start, r.on_end}) {
      pts.push_back(v);
      if (v > std::numeric_limits<int64_t>::min()) pts.push_back(v - 1);
      if (v < std::numeric_limits<int64_t>::max()) pts.push_back(v + 1);
    }
  pts.push_back(std::numeric_limits<int32_t>::min());
  pts.push_back(std::numeric_limits<int32_t>::max());
  if (pts.size() > 96) {  // (the 1024-range case: every 1 + size / 96-th point, the pairs stay affordable)
    std::vector<int64_t> few;
    const size_t step = 1 + pts.size() / 96;
    for (size_t i = 0; i < pts.size(); i += step) few.push_back(pts[i]);
    few.push_back(pts.back());
    pts.swap(few);
  }
  for (int op = RSET_INTERSECTS; op <= RSET_WITHIN; op++) {
    RangeSetTable t;
    if (!range_set_prepare(op, chrom.data(), bs.data(), be.data(), (int)ranges.size(), t)) {
      ok = false;
      break;
    }
    const size_t k = ranges.size();
    if (t.chrom.size() != k || t.key.size() != k || t.other.size() != k || t.agg.size() != k) ok = false;
    for (size_t i = 0; ok && i < k; i++) {
      if (i && (t.chrom[i - 1] > t.chrom[i] || (t.chrom[i - 1] == t.chrom[i] && t.key[i - 1] > t.key[i]))) ok = false;
      // the aggregate, from its definition: over the ranges of the SAME chromosome before (after) this one
      int64_t want = t.other[i];
      if (op == RSET_CONTAINS) {
        for (size_t j = i; j < k && t.chrom[j] == t.chrom[i]; j++) want = t.other[j] < want ? t.other[j] : want;
      } else {
        for (size_t j = i + 1; j-- > 0 && t.chrom[j] == t.chrom[i];) want = t.other[j] > want ? t.other[j] : want;
      }
      if (t.agg[i] != want) ok = false;
    }
    for (int32_t c : probe_chroms)
      for (int64_t s : pts)
        for (int64_t e : pts) {
          bool want = false;
          for (const Range& r : ranges) want = want || term(op, r, c, s, e);
          if (range_set_lookup(op, t, c, s, e) != want) {
            if (ok)
              fprintf(stderr, "%s: op %d chrom %d start %lld end %lld: want %d\n", name.c_str(), op, c, (long long)s,
                      (long long)e, (int)want);
            ok = false;
          }
        }
  }
  printf("%s range_set: %s\n", ok ? "ok  " : "FAIL", name.c_str());
  if (!ok) g_failed++;
}

int main() {
  const int64_t I64_MIN = std::numeric_limits<int64_t>::min(), I64_MAX = std::numeric_limits<int64_t>::max();
  check("one range", {{0, 100, 200}}, {-1, 0, 1});
  check("duplicate ranges", {{0, 100, 200}, {0, 100, 200}, {0, 100, 200}, {1, 5, 9}, {1, 5, 9}}, {0, 1, 2});
  // (INTERSECTS reads a range [lo, hi) as on_start = hi, on_end = lo; the other two as on_start = lo, on_end = hi)
  check("nested ranges", {{0, 1000, 0}, {0, 600, 400}, {0, 510, 490}, {0, 0, 1000}, {0, 400, 600}, {0, 490, 510}}, {0});
  check("a long range sorted well before the row's neighbours",
        {{0, 100000, 10}, {0, 530, 500}, {0, 630, 600}, {0, 730, 700}, {0, 830, 800}, {0, 10, 100000}}, {0}, {650, 660, 5000});
  check("a segment per chromosome", {{4, 10, 20}, {2, 10, 20}, {0, 10, 20}, {9, 10, 20}, {7, 30, 5}}, {0, 1, 2, 3, 4, 7, 9, 10});
  check("the aggregate does not leak across a chromosome boundary",
        {{0, 1000000, 0}, {0, 0, 1000000}, {1, 50, 40}, {1, 40, 50}, {2, 7, 3}}, {0, 1, 2}, {45, 500000});
  check("bounds at both ends of int64",
        {{0, I64_MIN, I64_MAX}, {0, I64_MAX, I64_MIN}, {1, I64_MIN, I64_MIN}, {1, I64_MAX, I64_MAX}, {2, I64_MAX - 1, I64_MIN + 1}},
        {0, 1, 2}, {0});
  {
    std::vector<Range> many;
    uint64_t x = 88172645463325252ull;
    for (int i = 0; i < RSET_MAX_RANGES; i++) {
      x ^= x << 13, x ^= x >> 7, x ^= x << 17;
      const int64_t lo = (int64_t)(x % 100000), len = 1 + (int64_t)((x >> 20) % 300);
      many.push_back({(int32_t)((x >> 40) % 5), i % 2 ? lo : lo + len, i % 2 ? lo + len : lo});
    }
    check("1024 ranges", many, {0, 1, 2, 3, 4, 5});
  }
  {
    RangeSetTable t;
    const int32_t c[1] = {0};
    const int64_t b[1] = {0};
    const bool refused = !range_set_prepare(RSET_INTERSECTS, c, b, b, 0, t) && !range_set_prepare(3, c, b, b, 1, t) &&
                         !range_set_prepare(RSET_WITHIN, c, b, b, RSET_MAX_RANGES + 1, t);
    printf("%s range_set: no ranges, too many and an unknown operator are refused\n", refused ? "ok  " : "FAIL");
    if (!refused) g_failed++;
  }
  if (g_failed) {
    printf("%d case(s) failed\n", g_failed);
    return 1;
  }
  printf("all cases passed\n");
  return 0;
}
