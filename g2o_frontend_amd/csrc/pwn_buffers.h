// pwn_buffers.h -- the owner of the library's own device and page-locked host memory: a pointer, a capacity in elements, and a
// destructor that frees.  Every workspace of pwn_hip_ctx and every array of a cloud -- its two sets of per-point arrays (CloudArrays), its size
// word, its index image -- is one of these, so that a buffer is named once (its member) and released without a list to keep in step; CloudDev
// and SceneBuffers are views of a cloud's owners, made for kernels and descriptors.  Not owned this way: what pwn_hip_device_alloc /
// pwn_hip_host_alloc hand to the caller.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>

namespace pwnhip {

enum class MemKind { Device, PinnedHost };

template <typename T, MemKind K>
struct Buf {
  T* p = nullptr;
  size_t cap = 0;                          // elements
  Buf() = default;
  Buf(const Buf&) = delete; Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  Buf& operator=(Buf&& o) noexcept { if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
  ~Buf() { release(); }
  operator T*() const { return p; }        // launch sites and pointer arithmetic read as with a plain pointer
  void release() { if (p) (void)(K == MemKind::Device ? hipFree(p) : hipHostFree(p)); p = nullptr; cap = 0; }
  // n elements for an EMPTY buffer
  hipError_t alloc(size_t n) {
    if (p) return hipErrorInvalidValue;
    const hipError_t e = K == MemKind::Device ? hipMalloc((void**)&p, n * sizeof(T)) : hipHostMalloc((void**)&p, n * sizeof(T));
    if (e == hipSuccess) cap = n; else p = nullptr;
    return e;
  }
  // at least n elements; the old block (and its content) goes when it is too small.  Never synchronises: where a stream may still use the
  // old block the caller waits for it first.
  hipError_t ensure(size_t n) { if (n <= cap) return hipSuccess; release(); return alloc(n); }
};
template <typename T> using DevBuf = Buf<T, MemKind::Device>;
template <typename T> using HostBuf = Buf<T, MemKind::PinnedHost>;

}  // namespace pwnhip
