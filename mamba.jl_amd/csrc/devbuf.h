// devbuf.h — DevBuf<T>: the one owner of a device allocation on the host side (engine.h).  Kept apart
// from engine.h so that it compiles without the kernel headers (tests/devbuf builds it against counting
// fakes of the HIP calls below).
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>

// Move-only; hipMalloc in alloc, hipFree in reset and the destructor.  Pinned: page-locked host memory
// (hipHostMalloc / hipHostFree) instead.  A group of buffers is dropped by assigning a fresh group.
template <class T, bool Pinned = false>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_;
      o.p_ = nullptr;
    }
    return *this;
  }
  ~DevBuf() { reset(); }
  // n elements, at least one (a buffer in use is never null); what was held is freed first
  hipError_t alloc(size_t n) {
    reset();
    const size_t nb = (n > 0 ? n : 1) * sizeof(T);
    const hipError_t st = Pinned ? hipHostMalloc((void**)&p_, nb, 0) : hipMalloc((void**)&p_, nb);
    if (st != hipSuccess) p_ = nullptr;
    return st;
  }
  hipError_t fill_bytes(int byte, size_t n) const { return hipMemset(p_, byte, n * sizeof(T)); }
  hipError_t zero(size_t n) const { return fill_bytes(0, n); }
  void reset() {
    if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
    p_ = nullptr;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }

 private:
  T* p_ = nullptr;
};
