// giql_amd/csrc/zero_ledger.h -- which bytes of the workspace are known to be zero, and how a call lays its workspace
// out.  Plain C++17, no HIP (tests/native/zero_ledger_check.cpp: without a GPU).
//
// A call that sorts zeroes everything its histograms and onesweep status words need at zero with ONE memset up front,
// and the helpers that would zero their own buffer (run_spans, run_linearize, run_sort_onesweep) skip theirs.  Whether
// a helper may skip is a fact about its BUFFER: it lies inside the range zeroed up front and nothing has written to it
// since.  The ledger records that range, and every buffer inside it that was handed to a writer.  A status word that is
// not zero sends the onesweep look-back after a predecessor that never ran, so every doubt resolves to "zero it again":
// slower, never wrong.
#pragma once

#include <cstddef>
#include <cstdint>

namespace giql {

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// [off, end) of the workspace, both 256-aligned: the part of a carve that is zeroed up front.
struct ZeroSpan {
  size_t off = 0, end = 0;
};

// Lays buffers out from `base`, each 256-aligned (base == nullptr: a dry run that only counts -- same offsets).
struct Carver {
  char* base;
  size_t off = 0;
  size_t zero_from = 0;
  template <typename T>
  T* take(size_t n) {
    off = align_up(off, 256);
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += n * sizeof(T);
    return p;
  }
  // everything taken between the two calls has to start at zero and lies back to back: one span, one memset
  void open_zeroed() { zero_from = off = align_up(off, 256); }
  ZeroSpan close_zeroed() {
    off = align_up(off, 256);
    return {zero_from, off};
  }
};

class ZeroLedger {
 public:
  static constexpr int MAX_TAKEN = 16;  // (the largest call takes fewer than ten buffers)

  // nothing is known to be zero
  void reset() {
    lo_ = hi_ = 0;
    n_taken_ = 0;
  }
  // the caller has enqueued its memset of [p, p + bytes): the range when there is none, its extension when p is the
  // range's end, and nothing otherwise (what is not recorded gets zeroed again)
  void add(const void* p, size_t bytes) {
    const uintptr_t q = reinterpret_cast<uintptr_t>(p);
    if (!p || bytes == 0) return;
    if (lo_ == hi_)
      lo_ = q, hi_ = q + bytes;
    else if (q == hi_)
      hi_ = q + bytes;
  }
  // [p, p + bytes) lies inside the range and touches no buffer taken so far
  bool covers(const void* p, size_t bytes) const {
    const uintptr_t q = reinterpret_cast<uintptr_t>(p);
    if (lo_ == hi_ || q < lo_ || q > hi_ || bytes > hi_ - q) return false;
    for (int i = 0; i < n_taken_; i++)
      if (q < taken_[i].hi && taken_[i].lo < q + bytes) return false;
    return true;
  }
  // true: the buffer is zero and now belongs to the caller, who skips its memset.  false: the caller zeroes it itself.
  // (A zero-byte buffer has nothing to zero and uses no entry.)
  bool take(const void* p, size_t bytes) {
    if (!covers(p, bytes)) return false;
    if (bytes == 0) return true;
    if (n_taken_ == MAX_TAKEN) return false;
    const uintptr_t q = reinterpret_cast<uintptr_t>(p);
    taken_[n_taken_++] = {q, q + bytes};
    return true;
  }
  // where the range ends (nullptr: there is none) -- for the caller that extends it
  const char* end() const { return reinterpret_cast<const char*>(hi_); }

 private:
  struct Taken {
    uintptr_t lo, hi;
  };
  uintptr_t lo_ = 0, hi_ = 0;
  int n_taken_ = 0;
  Taken taken_[MAX_TAKEN] = {};
};

}  // namespace giql
