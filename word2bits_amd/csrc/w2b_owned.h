// w2b_owned.h -- move-only owners of device memory, events and streams for the host side of the library (w2b_trainer.cpp,
// w2b_exchange.cpp).  Each converts to the raw handle it owns and releases it in its destructor.  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

// Device buffer of `cap` elements.  alloc() releases the old allocation first: the new one's contents are undefined.
template <class T>
struct W2bDevBuf {
  T *p = nullptr;
  size_t cap = 0;
  W2bDevBuf() = default;
  W2bDevBuf(W2bDevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  W2bDevBuf &operator=(W2bDevBuf &&o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
  ~W2bDevBuf() { (void)reset(); }
  hipError_t reset() { const hipError_t e = p ? hipFree(p) : hipSuccess; p = nullptr; cap = 0; return e; }
  hipError_t alloc(size_t n) {
    hipError_t e = reset();
    if (e == hipSuccess) e = hipMalloc(&p, sizeof(T) * n);
    if (e == hipSuccess) cap = n; else p = nullptr;
    return e;
  }
  operator T *() const { return p; }
  T *operator->() const { return p; }
};

template <class H, hipError_t (*Destroy)(H)>
struct W2bHandle {
  H h = nullptr;
  W2bHandle() = default;
  W2bHandle(W2bHandle &&o) noexcept : h(o.h) { o.h = nullptr; }
  W2bHandle &operator=(W2bHandle &&o) noexcept { std::swap(h, o.h); return *this; }
  ~W2bHandle() { if (h) (void)Destroy(h); }
  operator H() const { return h; }
};
struct W2bEvent : W2bHandle<hipEvent_t, hipEventDestroy> {
  hipError_t create(unsigned flags = hipEventDisableTiming) { return hipEventCreateWithFlags(&h, flags); }   // hipEventDefault: a timed one
};
struct W2bStream : W2bHandle<hipStream_t, hipStreamDestroy> {     // (destroying a stream does not wait for it: synchronise first)
  hipError_t create() { return hipStreamCreateWithFlags(&h, hipStreamNonBlocking); }
};
