// sweep.hip — the static instantiations of the block-sweep kernel (sweep.h) and their
// host-side launchers (line, rats, the node-IR interpreter).
#include "sweep.h"
#include "launch.h"
#include <cstdlib>

#ifdef MMB_PHASE_PROF
#include <cstdio>
__device__ unsigned long long mmb_prof[32];
void mmb_prof_dump() {
  unsigned long long h[32];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(mmb_prof), sizeof h) != hipSuccess) return;
  const char* names[] = {"amm:prep", "amm:load m/fl/Mv", "amm:proposal", "amm:logf x2+accept", "amm:moments+Sigma",
                         "amm:pchol", "amm:store", "gibbs", "iteration", "count", "pchol:steps",
                         "pchol:carry", "pchol:writeback", "amwg", "slice", "draws"};
  for (int i = 0; i < 16; ++i) fprintf(stderr, "MMB_PROF %-22s %llu\n", names[i], h[i]);
}
#endif

#ifdef MMB_WAVE_TIMES
#include <algorithm>
#include <cstdio>
#include <vector>
__device__ unsigned long long mmb_wt[3 * MMB_WT_MAX];
void mmb_wave_times_reset(hipStream_t st) {
  void* p = nullptr;
  if (hipGetSymbolAddress(&p, HIP_SYMBOL(mmb_wt)) == hipSuccess)
    (void)hipMemsetAsync(p, 0, sizeof(unsigned long long) * 3 * MMB_WT_MAX, st);
}
// occupancy of the last window's sweep launches, all parts: the window's span (first wave start
// to last wave end), the summed wave residency, and the fraction of the resident slots' time
// over that span which the waves filled
void mmb_wave_times_dump(int nwaves, int slots) {
  std::vector<unsigned long long> h(3 * MMB_WT_MAX);
  if (hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(mmb_wt), h.size() * sizeof(unsigned long long)) != hipSuccess) return;
  nwaves = std::min(nwaves, MMB_WT_MAX);
  unsigned long long t0 = ~0ull, t1 = 0;
  double busy = 0.0;
  int n = 0;
  for (int w = 0; w < nwaves; ++w) {
    if (h[3 * w] == 0 || h[3 * w + 1] < h[3 * w]) continue;
    t0 = std::min(t0, h[3 * w]);
    t1 = std::max(t1, h[3 * w + 1]);
    busy += (double)h[3 * w + 2];
    ++n;
  }
  if (!n) return;
  const double span = (double)(t1 - t0);
  fprintf(stderr, "MMB_WT window: wave slots %d span_us %.1f busy_per_slot_us %.1f fill(slots=%d) %.4f\n", n,
          span / 100.0, busy / n / 100.0, slots, busy / (span * slots));
}
#endif

// workgroups of the whole shard; a launch holds those of its part (SweepArgs wg_offset, wg_stride)
template <int MODEL, unsigned KINDS>
static hipError_t launch(const SweepArgs& A, hipStream_t st, int threads) {
  using M = Mdl<MODEL>;
  const int per_block = threads / M::G;
  const int nwg = (A.K + per_block - 1) / per_block;
  if (A.wg_stride < 1 || A.wg_offset < 0 || A.wg_offset >= A.wg_stride) return hipErrorInvalidValue;
  const int blocks = (nwg - A.wg_offset + A.wg_stride - 1) / A.wg_stride;
  if (blocks <= 0) return hipSuccess;  // a part past the last workgroup
  const size_t lds = (size_t)per_block * M::lds_stride(A) * sizeof(double);
  hipLaunchKernelGGL((sweep_kernel<MODEL, KINDS>), dim3(blocks), dim3(threads), lds, st, A);
  return hipGetLastError();
}

// launch shape of the shard: its workgroups and (wg_per_cu non-null) how many of them a CU holds at once
template <int MODEL, unsigned KINDS>
static hipError_t shape(const SweepArgs& A, int threads, int* nwg, int* wg_per_cu) {
  using M = Mdl<MODEL>;
  const int per_block = threads / M::G;
  *nwg = (A.K + per_block - 1) / per_block;
  if (!wg_per_cu) return hipSuccess;
  const size_t lds = (size_t)per_block * M::lds_stride(A) * sizeof(double);
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(wg_per_cu, sweep_kernel<MODEL, KINDS>, threads, lds);
}

// Wavefront pairing (engine.cpp order_chains): the slot -> chain table of the next window as a
// stable counting sort of the chains by class, on the engine stream right behind the previous
// window's last launch (no host round trip).  Class of chain k: per AMM block (the first block
// most significant, at most MMB_ORDER_BLOCKS of them), whether it holds a valid factor (flags
// bit 2).  One workgroup: thread t owns chains [t*C, (t+1)*C); the per-(class, thread) counts sit
// in LDS class-major, so one exclusive scan of that array gives every thread the first slot of
// its chains of each class, and chains of one class keep their index order.
constexpr int ORD_T = 1024;
constexpr int ORD_KC = 16384;  // shards up to this size read the flags once, coalesced, into LDS
__global__ __launch_bounds__(ORD_T) void order_chains_kernel(const OrderArgs a) {
  __shared__ int32_t cnt[(1 << MMB_ORDER_BLOCKS) * ORD_T];
  __shared__ int32_t wsum[ORD_T / 64];
  __shared__ uint8_t ccls[ORD_KC];
  const int t = (int)threadIdx.x;
  const int NC = 1 << a.nblk;
  const int C = (a.K + ORD_T - 1) / ORD_T;
  const int k0 = min(a.K, t * C), k1 = min(a.K, k0 + C);
  auto gcls = [&](int k) {
    int c = 0;
    for (int b = 0; b < a.nblk; ++b) c = (c << 1) | ((a.flags[b][k] >> 2) & 1);
    return c;
  };
  const bool cached = a.K <= ORD_KC;
  if (cached) {
    for (int k = t; k < a.K; k += ORD_T) ccls[k] = (uint8_t)gcls(k);
    __syncthreads();
  }
  auto cls = [&](int k) { return cached ? (int)ccls[k] : gcls(k); };
  for (int c = 0; c < NC; ++c) cnt[c * ORD_T + t] = 0;
  for (int k = k0; k < k1; ++k) cnt[cls(k) * ORD_T + t] += 1;
  __syncthreads();
  // exclusive scan of cnt[0 .. NC*T): thread t owns NC consecutive entries
  int* own = cnt + t * NC;
  int s = 0;
  for (int i = 0; i < NC; ++i) s += own[i];
  const int lane = t & 63, w = t >> 6;
  int inc = s;  // inclusive wave scan
  for (int d = 1; d < 64; d <<= 1) {
    const int v = __shfl_up(inc, d, 64);
    if (lane >= d) inc += v;
  }
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  int base = 0;
  for (int i = 0; i < w; ++i) base += wsum[i];
  int run = base + inc - s;
  __syncthreads();  // every thread has read the counts it owns before they are overwritten
  for (int i = 0; i < NC; ++i) {
    const int v = own[i];
    own[i] = run;
    run += v;
  }
  __syncthreads();
  // sorted position -> slot.  mode 1: reversed (slow classes dispatched first).  mode 2: the chain pairs of a wavefront stay consecutive in the
  // sorted order, but the W waves of a workgroup take their pairs from W different stretches of
  // it (pair q -> wave q / NF of workgroup q % NF, NF full workgroups), so every workgroup holds
  // fast and slow classes alike and the second dispatch round does not end on the slowest ones
  const int W = a.cpw / 2, NF = a.K / a.cpw;
  for (int k = k0; k < k1; ++k) {
    int* p = &cnt[cls(k) * ORD_T + t];
    int pos = *p;
    *p += 1;
    if (a.mode == 1) pos = a.K - 1 - pos;
    if (a.mode == 2 && W > 0 && (pos >> 1) < NF * W) {
      const int q = pos >> 1;
      pos = (q % NF) * a.cpw + 2 * (q / NF) + (pos & 1);
    }
    a.perm[pos] = k;
  }
}

hipError_t mmb_launch_order_chains(const OrderArgs& a, hipStream_t st) {
  if (a.nblk < 1 || a.nblk > MMB_ORDER_BLOCKS || a.K < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(order_chains_kernel, dim3(1), dim3(ORD_T), 0, st, a);
  return hipGetLastError();
}

// host-side launcher (engine.cpp); kinds = bitmask of the scheme's sampler kinds
hipError_t mmb_launch_sweep(int model, unsigned kinds, const SweepArgs& A, hipStream_t st) {
  if (model == MMB_MODEL_RATS) {
    constexpr int TB = MMB_RATS_BLOCK;
    if (kinds & K_RWM) return launch<MMB_MODEL_RATS, K_ALL | K_RWM>(A, st, TB);
    if ((kinds & ~K_GIBBS_AMM) == 0) return launch<MMB_MODEL_RATS, K_GIBBS_AMM>(A, st, TB);
    if ((kinds & ~K_SLICE_AMWG) == 0) return launch<MMB_MODEL_RATS, K_SLICE_AMWG>(A, st, TB);
    return launch<MMB_MODEL_RATS, K_ALL>(A, st, TB);
  }
  if (model == MMB_MODEL_IR) {
    if (kinds & K_ABC)
      return launch<MMB_MODEL_IR, K_IR | K_RWM | K_DGS | K_SIMPLEX | K_BIN | K_BHMC | K_ABC>(A, st, 128);
    if (kinds & K_BHMC) return launch<MMB_MODEL_IR, K_IR | K_RWM | K_DGS | K_SIMPLEX | K_BIN | K_BHMC>(A, st, 128);
    if (kinds & K_BIN) return launch<MMB_MODEL_IR, K_IR | K_RWM | K_DGS | K_SIMPLEX | K_BIN>(A, st, 128);
    if (kinds & K_SIMPLEX) return launch<MMB_MODEL_IR, K_IR | K_RWM | K_DGS | K_SIMPLEX>(A, st, 128);
    if (kinds & K_DGS) return launch<MMB_MODEL_IR, K_IR | K_RWM | K_DGS>(A, st, 128);
    if (kinds & K_RWM) return launch<MMB_MODEL_IR, K_IR | K_RWM>(A, st, 128);
    return launch<MMB_MODEL_IR, K_IR>(A, st, 128);
  }
  if (model == MMB_MODEL_LINE) {
    // one AMM block (BASELINE configs[1]): four lanes per chain, tune state in registers
    // (line_amm.hip); bit-identical to the generic kernel, which MMB_LINE_GENERIC=1 selects
    if (kinds == (1u << MMB_SAMPLER_AMM) && A.nb == 1 && !std::getenv("MMB_LINE_GENERIC"))
      return mmb_launch_line_amm(A, st);
    if (kinds & K_RWM) {
      if (kinds & K_GRAD) return launch<MMB_MODEL_LINE, K_ALL_GRAD | K_RWM>(A, st, 64);
      return launch<MMB_MODEL_LINE, K_ALL | K_RWM>(A, st, 64);
    }
    if (kinds & K_GRAD) return launch<MMB_MODEL_LINE, K_ALL_GRAD>(A, st, 64);
    return launch<MMB_MODEL_LINE, K_ALL>(A, st, 64);
  }
  return hipErrorInvalidValue;
}

// the 32-lane kernels' launch shape (engine.cpp sweep_parts); the same dispatch as mmb_launch_sweep
hipError_t mmb_sweep_shape(int model, unsigned kinds, const SweepArgs& A, int* nwg, int* wg_per_cu) {
  if (model == MMB_MODEL_RATS) {
    constexpr int TB = MMB_RATS_BLOCK;
    if (kinds & K_RWM) return shape<MMB_MODEL_RATS, K_ALL | K_RWM>(A, TB, nwg, wg_per_cu);
    if ((kinds & ~K_GIBBS_AMM) == 0) return shape<MMB_MODEL_RATS, K_GIBBS_AMM>(A, TB, nwg, wg_per_cu);
    if ((kinds & ~K_SLICE_AMWG) == 0) return shape<MMB_MODEL_RATS, K_SLICE_AMWG>(A, TB, nwg, wg_per_cu);
    return shape<MMB_MODEL_RATS, K_ALL>(A, TB, nwg, wg_per_cu);
  }
  if (model == MMB_MODEL_IR) {
    if (kinds & K_ABC)
      return shape<MMB_MODEL_IR, K_IR | K_RWM | K_DGS | K_SIMPLEX | K_BIN | K_BHMC | K_ABC>(A, 128, nwg, wg_per_cu);
    if (kinds & K_BHMC)
      return shape<MMB_MODEL_IR, K_IR | K_RWM | K_DGS | K_SIMPLEX | K_BIN | K_BHMC>(A, 128, nwg, wg_per_cu);
    if (kinds & K_BIN) return shape<MMB_MODEL_IR, K_IR | K_RWM | K_DGS | K_SIMPLEX | K_BIN>(A, 128, nwg, wg_per_cu);
    if (kinds & K_SIMPLEX) return shape<MMB_MODEL_IR, K_IR | K_RWM | K_DGS | K_SIMPLEX>(A, 128, nwg, wg_per_cu);
    if (kinds & K_DGS) return shape<MMB_MODEL_IR, K_IR | K_RWM | K_DGS>(A, 128, nwg, wg_per_cu);
    if (kinds & K_RWM) return shape<MMB_MODEL_IR, K_IR | K_RWM>(A, 128, nwg, wg_per_cu);
    return shape<MMB_MODEL_IR, K_IR>(A, 128, nwg, wg_per_cu);
  }
  return hipErrorInvalidValue;
}
