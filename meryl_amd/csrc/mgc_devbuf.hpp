// mgc_devbuf.hpp -- the one owning device buffer of the host code (everything but the session arena, the run store's records and
// pinned memory).  Internal.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>

namespace mgc {
// what the DBufs of this process hold (mgc_dev_buffers_live, mgc_api.cpp): relaxed, for tests and reports
struct DBufLive { std::atomic<uint64_t> bytes{0}, buffers{0}; };
inline DBufLive &dbuf_live() { static DBufLive l; return l; }

// Grow-only device buffer that frees itself.  Move-only; a moved-from or never-grown buffer is {nullptr, 0}.  It holds no device
// number and no stream: an owner that selects its device before freeing does so in its destructor body, which runs before the members go.
struct DBuf {
  void *p = nullptr; size_t cap = 0;
  DBuf() = default;
  DBuf(const DBuf &) = delete;
  DBuf &operator=(const DBuf &) = delete;
  DBuf(DBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  DBuf &operator=(DBuf &&o) noexcept {
    if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
    return *this;
  }
  ~DBuf() { release(); }
  hipError_t ensure(size_t bytes) {                        // no copy: what the buffer held is gone when it grows
    if (bytes < 256) bytes = 256;
    if (cap >= bytes) return hipSuccess;
    release();
    const hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) { p = nullptr; return e; }
    cap = bytes;
    dbuf_live().bytes.fetch_add(bytes, std::memory_order_relaxed);
    dbuf_live().buffers.fetch_add(1, std::memory_order_relaxed);
    return e;
  }
  void release() {
    if (!p) return;
    (void)hipFree(p);
    dbuf_live().bytes.fetch_sub(cap, std::memory_order_relaxed);
    dbuf_live().buffers.fetch_sub(1, std::memory_order_relaxed);
    p = nullptr; cap = 0;
  }
  template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};
}  // namespace mgc
