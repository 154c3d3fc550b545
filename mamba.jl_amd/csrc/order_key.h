// order_key.h -- the order-preserving 64-bit key of a double that the exact order statistics
// select on (summary.hip's radix-select histograms, diag.hip's per-thread select)
#ifndef MMB_ORDER_KEY_H
#define MMB_ORDER_KEY_H
#include <hip/hip_runtime.h>
#include <stdint.h>

// negative doubles reversed, positive ones above them
__device__ __forceinline__ uint64_t os_key(double x) {
  const uint64_t u = (uint64_t)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// the double of a key
__device__ __forceinline__ double os_unkey(uint64_t key) {
  return __longlong_as_double((long long)((key >> 63) ? key & 0x7fffffffffffffffull : ~key));
}

#endif
