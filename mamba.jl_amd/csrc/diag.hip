// diag.hip — per-chain convergence diagnostics of the device-kept draws.
//
// autocor / changerate (src/output/stats.jl:3-39), gewekediag (src/output/gewekediag.jl) and the
// :bm / :imse / :ipse MCSE estimators behind it (src/output/mcse.jl:10-46) are per-(chain, param)
// streaming reductions over a window [i0, i1) of one chain's kept draws.  The layout is
// summary.hip's: draws[(i*P + j)*K + k], one thread per (chain k, param j), adjacent threads =
// adjacent chains (coalesced), several independent loads in flight per thread.
//
// Centring (all kernels): the window mean is x[i0] + (sum of x - x[i0] in index order) / n_w and
// every sum of products is taken on z = x - mean.  A series whose elements are all equal gives
// z = 0 and gamma(l) = 0 exactly: mcse 0, autocorrelation 0/0 = NaN, Geweke z NaN, as the
// reference computes for a chain that never accepted.
//
// dg_autocov_kernel<NL>: gamma(l) = sum_t z_t z_{t+l} / n_w (StatsBase autocov, demean=true) at a
//   caller's lag list, all lags in ONE sweep: the leading stream x[t] is loaded once and each
//   lag has its own trailing stream x[t + l].
// dg_mcse_kernel<ETYPE>: batch means of the window alone (mcse_bm), or the initial monotone /
//   positive sequence estimators.  Their loop length depends on the data (tens to hundreds of
//   lag pairs), so the pairs are computed in blocks of DG_PAIRS: one sweep accumulates gamma for
//   2*DG_PAIRS consecutive lags from a register window of the leading stream, the min / break
//   rule of mcse.jl:27-31 / 40-44 is applied to the block afterwards, and only lanes whose rule
//   has not fired sweep again.  Where `value` is negative the reference's sqrt throws a
//   DomainError; the kernel writes NaN for that (chain, param).
// dg_change_kernel: changerate's counts.  One thread per chain; the inner loop over params keeps
//   the multivariate "any" in a register; per-param counts are summed per wavefront (ballot),
//   kept in LDS and flushed with 64-bit atomics.  Integer counts, exact.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mamba_hip.h"

#define DG_THREADS 64
#define DG_PAIRS 8                 // lag pairs per IMSE / IPSE sweep
#define DG_NLB (2 * DG_PAIRS)      // consecutive lags per sweep = register window length
#define DG_CH_U 8                  // rows per changerate step
#define DG_CH_MAXY 16
static_assert(DG_THREADS == 64, "dg_change_kernel sums one wavefront per workgroup with a ballot");

struct dg_lags {
  int64_t l[MMB_DIAG_MAX_LAGS];
};

// Loads are issued unconditionally (a row past the window's end is clamped to its last row and
// the value dropped by a select afterwards): a load under a per-lane branch is waited for inside
// the branch, which serialises the stream.
__device__ __forceinline__ double dg_ld(const double* __restrict__ p, size_t stride, int64_t r, int64_t i1) {
  return p[(size_t)(r < i1 ? r : i1 - 1) * stride];
}

// x[i0] and the window mean, summed on x - x[i0] in index order
__device__ __forceinline__ double dg_mean(const double* __restrict__ p, size_t stride, int64_t i0, int64_t i1) {
  constexpr int U = 16;
  const double x0 = p[(size_t)i0 * stride];
  double s = 0.0;
  for (int64_t t = i0; t < i1; t += U) {
    double xs[U];
#pragma unroll
    for (int u = 0; u < U; ++u) xs[u] = dg_ld(p, stride, t + u, i1);
#pragma unroll
    for (int u = 0; u < U; ++u) s += t + u < i1 ? xs[u] - x0 : 0.0;
  }
  return x0 + s / (double)(i1 - i0);
}

template <int NL>
__global__ __launch_bounds__(DG_THREADS) void dg_autocov_kernel(int P, int K, int64_t i0, int64_t i1, int nlags,
                                                               dg_lags lags, const double* __restrict__ draws,
                                                               double* __restrict__ out) {
  const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int j = (int)blockIdx.y;
  if (k >= K) return;
  const size_t stride = (size_t)P * K;
  const double* p = draws + (size_t)j * K + k;
  const double nw = (double)(i1 - i0);
  const double mean = dg_mean(p, stride, i0, i1);
  constexpr int U = NL <= 4 ? 8 : 4;
  double g0 = 0.0, acc[NL];
#pragma unroll
  for (int q = 0; q < NL; ++q) acc[q] = 0.0;
  for (int64_t t = i0; t < i1; t += U) {
    double a[U], b[NL][U];
#pragma unroll
    for (int u = 0; u < U; ++u) a[u] = dg_ld(p, stride, t + u, i1);
#pragma unroll
    for (int q = 0; q < NL; ++q)
      if (q < nlags) {
#pragma unroll
        for (int u = 0; u < U; ++u) b[q][u] = dg_ld(p, stride, t + u + lags.l[q], i1);
      }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      // past the window's end z counts as 0: the product adds nothing
      a[u] = t + u < i1 ? a[u] - mean : 0.0;
#pragma unroll
      for (int q = 0; q < NL; ++q) b[q][u] = (q < nlags && t + u + lags.l[q] < i1) ? b[q][u] - mean : 0.0;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      g0 = fma(a[u], a[u], g0);
#pragma unroll
      for (int q = 0; q < NL; ++q) acc[q] = fma(a[u], b[q][u], acc[q]);
    }
  }
  double* o = out + ((size_t)k * P + j) * (2 + nlags);
  o[0] = mean;
  o[1] = g0 / nw;
#pragma unroll
  for (int q = 0; q < NL; ++q)
    if (q < nlags) o[2 + q] = acc[q] / nw;
}

// mcse_bm(x; size=bs) of the window alone (mcse.jl:10-19): batches start at i0, remainder dropped
__device__ __forceinline__ void dg_bm(const double* __restrict__ p, size_t stride, int64_t i0, int64_t i1, int64_t bs,
                                      double mean, double* o) {
  constexpr int U = 16;
  const int64_t m = (i1 - i0) / bs;
  const double inv = 1.0 / (double)bs;
  double g0 = 0.0, acc = 0.0, b1 = 0.0, b2 = 0.0, d0 = 0.0;
  int64_t rem = bs, left = m;
  for (int64_t t = i0; t < i1; t += U) {
    double xs[U];
#pragma unroll
    for (int u = 0; u < U; ++u) xs[u] = dg_ld(p, stride, t + u, i1);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      xs[u] = t + u < i1 ? xs[u] - mean : 0.0;
      g0 = fma(xs[u], xs[u], g0);
      if (left > 0) {
        acc += xs[u];
        if (--rem == 0) {
          // batch means relative to the first one: equal batch means give a variance of 0
          // exactly, and the one-pass variance below loses nothing to a common offset
          if (left == m) d0 = acc * inv;
          const double d = acc * inv - d0;
          b1 += d;
          b2 = fma(d, d, b2);
          acc = 0.0;
          rem = bs;
          --left;
        }
      }
    }
  }
  // sem(mbar) = std(mbar) / sqrt(m), on the batch means of z less the first
  const double dm = (double)m;
  double var = (b2 - b1 * b1 / dm) / (dm - 1.0);
  if (var < 0.0) var = 0.0;
  o[1] = g0 / (double)(i1 - i0);
  o[2] = sqrt(var / dm);
  o[3] = dm;
}

// mcse_imse / mcse_ipse (mcse.jl:21-46) in blocks of DG_PAIRS lag pairs per sweep.  Pair i is
// (gamma(2i), gamma(2i+1)); pair 0 is the reference's `ghat = autocov(x, [0, 1])`.
template <int ETYPE>
__device__ __forceinline__ void dg_iseq(const double* __restrict__ p, size_t stride, int64_t i0, int64_t i1,
                                        double mean, double* o) {
  const int64_t n = i1 - i0;
  const double nw = (double)n;
  const int64_t m = (n - 2) / 2;             // div(n - 2, 2), n >= 2
  double Ghat = 0.0, value = 0.0, gam0 = 0.0, terms = 0.0;
  bool done = false;
  for (int64_t pair0 = 0; !done && pair0 <= m; pair0 += DG_PAIRS) {
    const int64_t L0 = 2 * pair0;            // this sweep: lags L0 .. L0 + DG_NLB - 1
    double acc[DG_NLB], w[DG_NLB];
#pragma unroll
    for (int q = 0; q < DG_NLB; ++q) {
      acc[q] = 0.0;
      w[q] = dg_ld(p, stride, i0 + L0 + q, i1);
    }
#pragma unroll
    for (int q = 0; q < DG_NLB; ++q) w[q] = i0 + L0 + q < i1 ? w[q] - mean : 0.0;
    // at step t the window holds z[t + L0 + q] in w[(t - i0 + q) % DG_NLB]; past the window's end
    // z counts as 0.  Lag L0 has terms for t < i1 - L0; the longer lags meet the zeros earlier.
    const int64_t tend = i1 - L0;
    for (int64_t t = i0; t < tend; t += DG_NLB) {
      double a[DG_NLB], nx[DG_NLB];
#pragma unroll
      for (int u = 0; u < DG_NLB; ++u) {
        a[u] = dg_ld(p, stride, t + u, i1);
        nx[u] = dg_ld(p, stride, t + u + L0 + DG_NLB, i1);
      }
#pragma unroll
      for (int u = 0; u < DG_NLB; ++u) {
        a[u] = t + u < tend ? a[u] - mean : 0.0;
        nx[u] = t + u + L0 + DG_NLB < i1 ? nx[u] - mean : 0.0;
      }
#pragma unroll
      for (int u = 0; u < DG_NLB; ++u) {
#pragma unroll
        for (int q = 0; q < DG_NLB; ++q) acc[q] = fma(a[u], w[(u + q) % DG_NLB], acc[q]);
        w[u] = nx[u];
      }
    }
#pragma unroll
    for (int r = 0; r < DG_PAIRS; ++r) {
      const int64_t i = pair0 + r;
      if (!done && i <= m) {
        const double ga = acc[2 * r] / nw, gb = acc[2 * r + 1] / nw;
        if (i == 0) {
          gam0 = ga;
          if (ETYPE == MMB_MCSE_IMSE) {
            Ghat = ga + gb;
            value = -ga + 2.0 * Ghat;
          } else {
            value = ga + 2.0 * gb;
          }
        } else {
          const double s = ga + gb;
          if (ETYPE == MMB_MCSE_IMSE) {
            if (s < Ghat || s != s) Ghat = s;   // min(Ghat, s), NaN kept as Julia's min does
          } else {
            Ghat = s;
          }
          if (Ghat > 0.0) {
            value += 2.0 * Ghat;
            terms += 1.0;
          } else {
            done = true;                        // Ghat > 0 || break
          }
        }
      }
    }
  }
  o[1] = gam0;
  o[2] = sqrt(value / nw);                      // value < 0 (reference: DomainError) -> NaN
  o[3] = terms;
}

template <int ETYPE>
__global__ __launch_bounds__(DG_THREADS) void dg_mcse_kernel(int P, int K, int64_t i0, int64_t i1, int64_t bs,
                                                            const double* __restrict__ draws,
                                                            double* __restrict__ out) {
  const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int j = (int)blockIdx.y;
  if (k >= K) return;
  const size_t stride = (size_t)P * K;
  const double* p = draws + (size_t)j * K + k;
  double* o = out + ((size_t)k * P + j) * MMB_MCSE_FIELDS;
  const double mean = dg_mean(p, stride, i0, i1);
  o[0] = mean;
  if (ETYPE == MMB_MCSE_BM) dg_bm(p, stride, i0, i1, bs, mean, o);
  else dg_iseq<ETYPE>(p, stride, i0, i1, mean, o);
}

// changerate (stats.jl:19-39): blockIdx.y takes a contiguous run of rows; the counts add up.
__global__ __launch_bounds__(DG_THREADS) void dg_change_kernel(int P, int K, int64_t n, int64_t rows_per_y,
                                                              const double* __restrict__ draws,
                                                              unsigned long long* __restrict__ out) {
  extern __shared__ unsigned long long dg_cnt[];   // P per-param counts of this wavefront + "any"
  for (int q = threadIdx.x; q <= P; q += blockDim.x) dg_cnt[q] = 0ull;
  __syncthreads();
  const int kk = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const bool live = kk < K;
  const int k = live ? kk : K - 1;                 // idle lanes stay in the wavefront for the ballots
  const size_t stride = (size_t)P * K;
  const int64_t r0 = 1 + (int64_t)blockIdx.y * rows_per_y;
  const int64_t r1 = r0 + rows_per_y < n ? r0 + rows_per_y : n;
  unsigned long long mv = 0ull;
  for (int64_t i = r0; i < r1; i += DG_CH_U) {
    unsigned any = 0u;
    for (int j = 0; j < P; ++j) {
      const double* p = draws + (size_t)j * K + k;
      double xs[DG_CH_U + 1];
#pragma unroll
      for (int u = 0; u <= DG_CH_U; ++u) {
        const int64_t r = i - 1 + u;
        xs[u] = p[(size_t)(r < r1 ? r : r1 - 1) * stride];
      }
      unsigned c = 0u;
#pragma unroll
      for (int u = 0; u < DG_CH_U; ++u) {
        const bool dx = live && i + u < r1 && xs[u + 1] != xs[u];
        any |= dx ? 1u << u : 0u;
        c += (unsigned)__popcll(__ballot(dx));
      }
      if (threadIdx.x == 0) dg_cnt[j] += c;
    }
    mv += (unsigned)__popc(any);
  }
  if (mv) atomicAdd(&dg_cnt[P], mv);
  __syncthreads();
  for (int q = threadIdx.x; q <= P; q += blockDim.x)
    if (dg_cnt[q]) atomicAdd(&out[q], dg_cnt[q]);
}

hipError_t mmb_launch_chain_autocov(int P, int K, int64_t i0, int64_t i1, int nlags, const int64_t* lags,
                                    const double* draws, double* out, hipStream_t st) {
  if (nlags < 0 || nlags > MMB_DIAG_MAX_LAGS || i0 < 0 || i1 <= i0) return hipErrorInvalidValue;
  dg_lags L;
  for (int q = 0; q < MMB_DIAG_MAX_LAGS; ++q) L.l[q] = q < nlags ? lags[q] : 1;
  const dim3 grid((K + DG_THREADS - 1) / DG_THREADS, P), blk(DG_THREADS);
  if (nlags <= 4) hipLaunchKernelGGL(dg_autocov_kernel<4>, grid, blk, 0, st, P, K, i0, i1, nlags, L, draws, out);
  else hipLaunchKernelGGL(dg_autocov_kernel<MMB_DIAG_MAX_LAGS>, grid, blk, 0, st, P, K, i0, i1, nlags, L, draws, out);
  return hipGetLastError();
}

hipError_t mmb_launch_chain_mcse(int P, int K, int64_t i0, int64_t i1, int etype, int64_t bs, const double* draws,
                                 double* out, hipStream_t st) {
  if (i0 < 0 || i1 <= i0) return hipErrorInvalidValue;
  const dim3 grid((K + DG_THREADS - 1) / DG_THREADS, P), blk(DG_THREADS);
  if (etype == MMB_MCSE_BM) {
    if (bs < 1 || (i1 - i0) / bs < 2) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dg_mcse_kernel<MMB_MCSE_BM>, grid, blk, 0, st, P, K, i0, i1, bs, draws, out);
  } else if (etype == MMB_MCSE_IMSE || etype == MMB_MCSE_IPSE) {
    if (i1 - i0 < 2) return hipErrorInvalidValue;
    if (etype == MMB_MCSE_IMSE)
      hipLaunchKernelGGL(dg_mcse_kernel<MMB_MCSE_IMSE>, grid, blk, 0, st, P, K, i0, i1, bs, draws, out);
    else
      hipLaunchKernelGGL(dg_mcse_kernel<MMB_MCSE_IPSE>, grid, blk, 0, st, P, K, i0, i1, bs, draws, out);
  } else {
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// out: P + 1 counts (device), zeroed here
hipError_t mmb_launch_change_counts(int P, int K, int64_t n, const double* draws, unsigned long long* out,
                                    hipStream_t st) {
  hipError_t e = hipMemsetAsync(out, 0, (size_t)(P + 1) * sizeof(unsigned long long), st);
  if (e != hipSuccess || n < 2) return e;
  // rows 1 .. n-1 in up to DG_CH_MAXY runs of whole DG_CH_U steps: enough wavefronts to fill the
  // device at a few thousand chains without shortening each thread's stream below a few steps
  int64_t ny = (n - 1 + 4 * DG_CH_U - 1) / (4 * DG_CH_U);
  if (ny > DG_CH_MAXY) ny = DG_CH_MAXY;
  int64_t per = (n - 1 + ny - 1) / ny;
  per = (per + DG_CH_U - 1) / DG_CH_U * DG_CH_U;
  ny = (n - 1 + per - 1) / per;
  const dim3 grid((K + DG_THREADS - 1) / DG_THREADS, (unsigned)ny), blk(DG_THREADS);
  hipLaunchKernelGGL(dg_change_kernel, grid, blk, (size_t)(P + 1) * sizeof(unsigned long long), st, P, K, n, per,
                     draws, out);
  return hipGetLastError();
}
