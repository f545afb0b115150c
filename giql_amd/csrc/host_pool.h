// giql_amd/csrc/host_pool.h -- the pool behind the library-owned host outputs (host_alloc / giql_hip_free_host in
// giql_hip.hip).  Page-locking is the expensive part of the PCIe-inclusive calls -- 3.2 GB of pairs: 203 ms to pin,
// 57 ms to copy (GIQL_HIP_DEBUG_E2E=1) -- so released buffers are kept for the next call: best fit, at most
// `idle_limit` bytes of idle memory.  Plain C++17, no HIP: the two functions that allocate and release page-locked
// memory are handed in (giql_hip.hip: hipHostMalloc / hipHostFree; tests/native/host_side_check.cpp: a counting fake).
#pragma once

#include <sys/mman.h>

#include <cstdlib>
#include <mutex>
#include <vector>

class HostPool {
 public:
  using PinnedAlloc = void* (*)(size_t bytes);  // nullptr when there is no memory
  using PinnedFree = void (*)(void* p);

  HostPool(size_t idle_limit, PinnedAlloc pinned_alloc, PinnedFree pinned_free)
      : idle_limit_(idle_limit), pinned_alloc_(pinned_alloc), pinned_free_(pinned_free) {}

  // at least `bytes` (0 counts as 1) of page-locked or plain memory (outputs that host threads write); nullptr: no memory
  void* get(size_t bytes, bool pinned = true) {
    if (bytes == 0) bytes = 1;
    {
      std::lock_guard<std::mutex> g(mu_);
      Buf* best = nullptr;
      for (auto& b : bufs_)  // (a page-locked buffer serves a plain request as well)
        if (b.idle && b.bytes >= bytes && (b.pinned || !pinned) && (!best || b.bytes < best->bytes)) best = &b;
      if (best && best->bytes <= 2 * bytes + (1u << 20)) {  // not a 3 GB buffer for a 4-byte result
        best->idle = false;
        return best->p;
      }
    }
    void* p = nullptr;
    size_t cap = bytes + bytes / 16;  // a little head-room: the next result of a similar call fits too
    if (pinned) {
      p = pinned_alloc_(cap);
      if (!p) return nullptr;
    } else {
      // plain memory on 2 MiB boundaries, huge pages asked for: the expansion threads touch it for the first time
      // (4 KB pages: ~800,000 faults for 3.2 GB of pairs)
      constexpr size_t HUGE_PAGE = (size_t)2 << 20;
      cap = (cap + HUGE_PAGE - 1) / HUGE_PAGE * HUGE_PAGE;
      p = aligned_alloc(HUGE_PAGE, cap);
      if (!p) return nullptr;
#if defined(MADV_HUGEPAGE)
      (void)madvise(p, cap, MADV_HUGEPAGE);
#endif
    }
    std::lock_guard<std::mutex> g(mu_);
    bufs_.push_back({p, cap, false, pinned});
    return p;
  }

  // (a pointer the pool does not know is released as page-locked memory)
  void put(void* p) {
    bool known = false;
    {
      std::lock_guard<std::mutex> g(mu_);
      for (auto& b : bufs_)
        if (b.p == p) b.idle = known = true;
    }
    if (!known) pinned_free_(p);
    (void)release_idle(idle_limit_, false);  // the smallest first: the big ones are the ones worth keeping
  }

  // releases idle buffers, the smallest or the largest first, until at most `keep_bytes` are idle; returns the bytes released
  size_t release_idle(size_t keep_bytes, bool largest_first) {
    std::vector<Buf> drop;
    size_t freed = 0;
    {
      std::lock_guard<std::mutex> g(mu_);
      size_t idle = 0;
      for (auto& b : bufs_)
        if (b.idle) idle += b.bytes;
      while (idle > keep_bytes) {
        size_t k = bufs_.size();
        for (size_t i = 0; i < bufs_.size(); i++)
          if (bufs_[i].idle &&
              (k == bufs_.size() || (largest_first ? bufs_[i].bytes > bufs_[k].bytes : bufs_[i].bytes < bufs_[k].bytes)))
            k = i;
        if (k == bufs_.size()) break;
        idle -= bufs_[k].bytes;
        freed += bufs_[k].bytes;
        drop.push_back(bufs_[k]);
        bufs_.erase(bufs_.begin() + (long)k);
      }
    }
    for (auto& d : drop) d.pinned ? pinned_free_(d.p) : free(d.p);  // (outside the lock)
    return freed;
  }

 private:
  struct Buf {
    void* p;
    size_t bytes;
    bool idle;
    bool pinned;
  };
  std::mutex mu_;
  std::vector<Buf> bufs_;
  const size_t idle_limit_;
  const PinnedAlloc pinned_alloc_;
  const PinnedFree pinned_free_;
};
