// hip_own.hpp -- device memory, pinned memory, events and streams that free themselves.  Host code only, no kernels.
// All four are move-only and have the same shape: public members, release(), creation that returns the hipError_t (the
// caller keeps its own error macro).  Each is freed on the device that is current when it dies: hipSetDevice first.
#pragma once
#include <hip/hip_runtime_api.h>

struct DBuf {  // grow-only device buffer; owns its memory (freed on the device that is current when it dies: hipSetDevice first)
  void *p = nullptr;
  size_t cap = 0;
  DBuf() = default;
  DBuf(DBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  DBuf &operator=(DBuf &&o) noexcept { if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
  ~DBuf() { release(); }
  void release() { if (p) hipFree(p); p = nullptr; cap = 0; }
  template <typename T> T *as() const { return static_cast<T *>(p); }
};
static_assert(!std::is_copy_constructible<DBuf>::value && !std::is_copy_assignable<DBuf>::value, "a DBuf is handed over with std::move");
// a fresh block of exactly `bytes` for the code that does not grow its buffers; what d held goes first
inline hipError_t dbuf_alloc(DBuf &d, size_t bytes) {
  d.release();
  const hipError_t e = hipMalloc(&d.p, bytes);
  if (e == hipSuccess) d.cap = bytes; else d.p = nullptr;
  return e;
}

struct HBuf {  // pinned host buffer that knows its size
  void *p = nullptr;
  size_t cap = 0;
  HBuf() = default;
  HBuf(HBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  HBuf &operator=(HBuf &&o) noexcept { if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
  ~HBuf() { release(); }
  hipError_t alloc(size_t bytes) {
    release();
    const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
    if (e == hipSuccess) cap = bytes; else p = nullptr;
    return e;
  }
  void release() { if (p) hipHostFree(p); p = nullptr; cap = 0; }
  template <typename T> T *as() const { return static_cast<T *>(p); }
};

struct Event {  // without timing unless asked for
  hipEvent_t e = nullptr;
  Event() = default;
  Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
  Event &operator=(Event &&o) noexcept { if (this != &o) { release(); e = o.e; o.e = nullptr; } return *this; }
  ~Event() { release(); }
  hipError_t create(bool timing = false) { release(); return timing ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, hipEventDisableTiming); }
  void release() { if (e) hipEventDestroy(e); e = nullptr; }
  operator hipEvent_t() const { return e; }
};

struct Stream {  // non-blocking
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(Stream &&o) noexcept : s(o.s) { o.s = nullptr; }
  Stream &operator=(Stream &&o) noexcept { if (this != &o) { release(); s = o.s; o.s = nullptr; } return *this; }
  ~Stream() { release(); }
  hipError_t create() { release(); return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
  void release() { if (s) hipStreamDestroy(s); s = nullptr; }
  operator hipStream_t() const { return s; }
};
