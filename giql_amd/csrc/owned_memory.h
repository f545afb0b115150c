// giql_amd/csrc/owned_memory.h -- the two owners of the memory giql_hip.hip allocates: a device buffer (hipMalloc /
// hipFree) and a pointer from the pinned-host pool (host_pool.h, through host_alloc / giql_hip_free_host).  Both are move-only and release
// what they hold when they go out of scope, so an early return needs no clean-up of its own.  Included by
// giql_hip.hip after set_err / HIP_TRY, which it reports through.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/giql_hip.h"

// A device buffer and the bytes it was asked for.
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr, o.bytes_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_, bytes_ = o.bytes_;
      o.p_ = nullptr, o.bytes_ = 0;
    }
    return *this;
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { reset(); }

  void* get() const { return p_; }
  size_t bytes() const { return bytes_; }

  // exactly `bytes` (whatever the buffer held is released first)
  int alloc(size_t bytes) {
    reset();
    HIP_TRY(hipMalloc(&p_, bytes));
    bytes_ = bytes;
    return GIQL_OK;
  }

  // Grown on demand: at least `need` bytes, `want` of them when it has to grow (the buffer's slack).  The old buffer
  // may still be read by work on `stream`; it is freed after that work.
  int grow(size_t need, size_t want, hipStream_t stream, const char* what) {
    if (need <= bytes_) return GIQL_OK;
    HIP_TRY(hipStreamSynchronize(stream));
    if (p_) HIP_TRY(hipFree(p_));
    p_ = nullptr;
    bytes_ = 0;
    const hipError_t e = hipMalloc(&p_, want);
    if (e != hipSuccess)
      return set_err(GIQL_ERR_NOMEM, "hipMalloc(%zu bytes) for %s failed: %s", want, what, hipGetErrorString(e));
    bytes_ = want;
    return GIQL_OK;
  }

  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr, bytes_ = 0;
  }

 private:
  void* p_ = nullptr;
  size_t bytes_ = 0;
};

// The buffer as an array of T: reads as the T* it replaces (kernel arguments, pointer arithmetic, tests against NULL).
template <typename T>
struct DevArray : DevBuf {
  operator T*() const { return static_cast<T*>(get()); }
  T* operator->() const { return static_cast<T*>(get()); }
};

// A pointer from the host pool (host_alloc), back to the pool when its owner goes.
template <typename T>
class HostPtr {
 public:
  explicit HostPtr(void* p = nullptr) : p_(static_cast<T*>(p)) {}
  HostPtr(HostPtr&& o) noexcept : p_(o.release()) {}
  HostPtr& operator=(HostPtr&& o) noexcept {
    if (this != &o) {
      giql_hip_free_host(p_);
      p_ = o.release();
    }
    return *this;
  }
  HostPtr(const HostPtr&) = delete;
  HostPtr& operator=(const HostPtr&) = delete;
  ~HostPtr() { giql_hip_free_host(p_); }

  operator T*() const { return p_; }
  T* release() {  // the pointer leaves through the C ABI: the caller frees it with giql_hip_free_host
    T* p = p_;
    p_ = nullptr;
    return p;
  }

 private:
  T* p_;
};
