// Counting fakes of the HIP calls csrc/devbuf.h makes, found in place of the runtime's header when
// devbuf_test.cpp is built with -I tests/devbuf.  Host memory stands in for device memory, so the
// sanitizers see every allocation, a leak, a double free and a use after free.
#pragma once
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

typedef int hipError_t;
#define hipSuccess 0
#define hipErrorOutOfMemory 2

struct FakeHip {
  long mallocs = 0, frees = 0, host_mallocs = 0, host_frees = 0, memsets = 0;
  size_t last_bytes = 0;
  bool fail_next = false;  // the next allocation reports out of memory
};
inline FakeHip& fake_hip() {
  static FakeHip f;
  return f;
}

inline hipError_t fake_alloc(void** p, size_t nb, long& count) {
  FakeHip& f = fake_hip();
  if (f.fail_next) {
    f.fail_next = false;
    return hipErrorOutOfMemory;  // (leaves *p alone, as the runtime may)
  }
  *p = malloc(nb);
  f.last_bytes = nb;
  ++count;
  return hipSuccess;
}
inline hipError_t hipMalloc(void** p, size_t nb) { return fake_alloc(p, nb, fake_hip().mallocs); }
inline hipError_t hipHostMalloc(void** p, size_t nb, unsigned) { return fake_alloc(p, nb, fake_hip().host_mallocs); }
inline hipError_t hipFree(void* p) {
  free(p);
  ++fake_hip().frees;
  return hipSuccess;
}
inline hipError_t hipHostFree(void* p) {
  free(p);
  ++fake_hip().host_frees;
  return hipSuccess;
}
inline hipError_t hipMemset(void* p, int v, size_t nb) {
  memset(p, v, nb);
  ++fake_hip().memsets;
  return hipSuccess;
}
