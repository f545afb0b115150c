// giql_amd/csrc/range_set_prepare.h -- the host half of giql_hip_range_set_any_dev: one set of literal ranges, as the
// caller hands it over (any order, duplicates allowed), becomes the table the kernel searches.  Plain C++17, no HIP
// (tests/native/range_set_check.cpp: without a GPU).
//
// `col <op> ANY(r_1 .. r_K)` is an OR of K terms  chrom = c AND <cmp on start> AND <cmp on end>.  With the ranges of
// one chromosome ordered by the bound of ONE of the two comparisons, the rows that pass that comparison against a
// range form a prefix (or a suffix) of the order, found by one binary search; whether any range of that prefix passes
// the OTHER comparison is one look at a running maximum (minimum) of the other bound.  The aggregate restarts at
// every chromosome.  bs / be are the bounds on the raw `start` / `end` columns:
//
//   op          term                       key (order)   other   aggregate           a row (start, end) matches when
//   INTERSECTS  start <  bs AND end >  be   be            bs      prefix max(other)   agg[#{key <  end}   - 1] >  start
//   WITHIN      start >= bs AND end <= be   bs            be      prefix max(other)   agg[#{key <= start} - 1] >= end
//   CONTAINS    start <= bs AND end >= be   bs            be      suffix min(other)   agg[first key >= start]  <= end
//
// Nothing is added to or subtracted from a bound here: the caller has moved the table's encoding onto them already,
// and a bound at either end of int64 is compared like any other.
#pragma once

#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

namespace giql {

constexpr int RSET_INTERSECTS = 0, RSET_CONTAINS = 1, RSET_WITHIN = 2;  // GIQL_RANGE_* of the C ABI
constexpr int RSET_MAX_RANGES = 1024;  // ranges per set (the kernel's LDS table)
constexpr int RSET_MAX_SETS = 8;       // sets per call

struct RangeSetTable {  // the K ranges ordered by (chrom, key)
  std::vector<int32_t> chrom;
  std::vector<int64_t> key, other, agg;
};

// false: an unknown op or k outside [1, RSET_MAX_RANGES] (nothing is written then)
inline bool range_set_prepare(int op, const int32_t* chrom, const int64_t* on_start, const int64_t* on_end, int k,
                              RangeSetTable& t) {
  if (op < RSET_INTERSECTS || op > RSET_WITHIN || k < 1 || k > RSET_MAX_RANGES || !chrom || !on_start || !on_end)
    return false;
  const int64_t* key = op == RSET_INTERSECTS ? on_end : on_start;
  const int64_t* other = op == RSET_INTERSECTS ? on_start : on_end;
  std::vector<int> order((size_t)k);
  std::iota(order.begin(), order.end(), 0);
  std::sort(order.begin(), order.end(), [&](int a, int b) {
    if (chrom[a] != chrom[b]) return chrom[a] < chrom[b];
    if (key[a] != key[b]) return key[a] < key[b];
    if (other[a] != other[b]) return other[a] < other[b];
    return a < b;
  });
  t.chrom.resize((size_t)k);
  t.key.resize((size_t)k);
  t.other.resize((size_t)k);
  t.agg.resize((size_t)k);
  for (int i = 0; i < k; i++) {
    t.chrom[i] = chrom[order[i]];
    t.key[i] = key[order[i]];
    t.other[i] = other[order[i]];
  }
  if (op == RSET_CONTAINS) {
    for (int i = k - 1; i >= 0; i--) {
      const bool first = i == k - 1 || t.chrom[i + 1] != t.chrom[i];  // (the last range of its chromosome)
      t.agg[i] = first ? t.other[i] : std::min(t.other[i], t.agg[i + 1]);
    }
  } else {
    for (int i = 0; i < k; i++) {
      const bool first = i == 0 || t.chrom[i - 1] != t.chrom[i];
      t.agg[i] = first ? t.other[i] : std::max(t.other[i], t.agg[i - 1]);
    }
  }
  return true;
}

// The answer for one row without NULLs, from the table alone: what the kernel computes per row, restated for the
// stand-alone check (one binary search on (chrom, key), one compare with the aggregate).
inline bool range_set_lookup(int op, const RangeSetTable& t, int32_t c, int64_t start, int64_t end) {
  const int k = (int)t.chrom.size();
  const int64_t probe = op == RSET_INTERSECTS ? end : start;
  int lo = 0, hi = k;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const bool below = t.chrom[mid] < c ||
                       (t.chrom[mid] == c && (op == RSET_WITHIN ? t.key[mid] <= probe : t.key[mid] < probe));
    if (below)
      lo = mid + 1;
    else
      hi = mid;
  }
  if (op == RSET_CONTAINS) return lo < k && t.chrom[lo] == c && t.agg[lo] <= end;
  if (lo == 0 || t.chrom[lo - 1] != c) return false;
  return op == RSET_INTERSECTS ? t.agg[lo - 1] > start : t.agg[lo - 1] >= end;
}

}  // namespace giql
