// esa_own.h -- the owners of what the library gets from the HIP runtime and the
// loader: device memory, pinned host memory, streams, events, dlopen handles.
// The only calls that create or release one of these are in this file; an owner
// releases what it holds when it goes away, so that a frame left early (HIP_TRY,
// TRY, an exception on its way to GTAMD_ABI_END) leaks nothing.  hipFree waits
// for the device: releasing memory behind kernels still in flight is safe.
// Nothing here words an error: creation hands back a status.
#pragma once
#include <dlfcn.h>
#include "esa_common.h"

// move-only holder of one handle that `Release` gives back
template <typename H, typename Release> struct Owned {
  H h = H();
  Owned() = default;
  Owned(Owned &&o) noexcept : h(o.h) { o.h = H(); }
  Owned &operator=(Owned &&o) noexcept {
    if (this != &o) { reset(); h = o.h; o.h = H(); }
    return *this;
  }
  ~Owned() { reset(); }
  void reset() { if (h != H()) Release()(h); h = H(); }
  operator H() const { return h; }
};

struct ReleaseStream { void operator()(hipStream_t s) const { (void) hipStreamDestroy(s); } };
struct ReleaseEvent { void operator()(hipEvent_t e) const { (void) hipEventDestroy(e); } };
struct ReleaseLib { void operator()(void *l) const { (void) dlclose(l); } };
typedef Owned<hipStream_t, ReleaseStream> Stream;
typedef Owned<hipEvent_t, ReleaseEvent> Event;
typedef Owned<void *, ReleaseLib> SharedLib;

static inline hipError_t create(Stream &s, unsigned flags = hipStreamDefault) {
  s.reset();
  return hipStreamCreateWithFlags(&s.h, flags);
}
static inline hipError_t create(Event &e, unsigned flags = hipEventDefault) {
  e.reset();
  return hipEventCreateWithFlags(&e.h, flags);
}
static inline bool open_lib(SharedLib &l, const char *name) {
  l.reset();
  l.h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
  return l.h != nullptr;
}

// device memory, or (PINNED) page-locked host memory
template <bool PINNED> struct Mem {
  void *p = nullptr;
  u64 bytes = 0;
  Mem() = default;
  Mem(Mem &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
  Mem &operator=(Mem &&o) noexcept {
    if (this != &o) { reset(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
    return *this;
  }
  ~Mem() { reset(); }
  template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
  void reset() {
    if (p != nullptr) (void) (PINNED ? hipHostFree(p) : hipFree(p));
    p = nullptr; bytes = 0;
  }
  // exactly n bytes; what was there is dropped first
  hipError_t alloc(u64 n) {
    reset();
    const hipError_t e = PINNED ? hipHostMalloc(&p, n, hipHostMallocDefault) : hipMalloc(&p, n);
    if (e != hipSuccess) p = nullptr;
    else bytes = n;
    return e;
  }
  // at least n bytes; growing loses the contents
  hipError_t grow(u64 n) { return n <= bytes ? hipSuccess : alloc(n); }
};
typedef Mem<false> DevBuf;

// the same, read as an array of T where a T* is wanted
template <typename T, bool PINNED = false> struct Array : Mem<PINNED> {
  operator T *() const { return reinterpret_cast<T *>(this->p); }
  T *operator->() const { return reinterpret_cast<T *>(this->p); }
};
template <typename T> using Dev = Array<T, false>;
template <typename T> using Pinned = Array<T, true>;
