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
#include "mmb_math.h"
#include "order_key.h"
#include "launch.h"

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

// ---- Heidelberger-Welch and Raftery-Lewis partials (heideldiag.jl:3-27, rafterydiag.jl:3-47)
//
// dg_cvm_kernel<NS>: the Cramer-von Mises sums of heideldiag.jl:11-16 for every candidate window
//   [s_q, n) of one series in two sweeps over the rows from s_0 on.  Sweep 1 takes the sums of
//   x - x[s_0] in index order and adds each segment [s_q, s_{q+1}) to the suffix sums of the
//   starts at or before it: mean_q = x[s_0] + suffix_q / m_q.  Sweep 2 keeps a running (B, sum B^2)
//   per start whose window has begun, B accumulated on the centred values z = x - mean_q, so a
//   series of equal elements gives W = 0 exactly.  W_q = sum B^2 / m_q^2; the 1 / S0 stays on the host.
// dg_mcse_from_kernel<ETYPE>: dg_mcse_kernel with the window start read per (chain, param); the
//   same device functions, so equal starts give the same bits.
// dg_raftery_kernel: the threshold quantile(x, q) by an exact per-thread select on the
//   order-preserving key (most significant digit first, DG_RF_BITS bits per sweep, the
//   cumulative digit counters in registers), then the thinning loop of rafterydiag.jl:17-33 on
//   dichot = x <= threshold evaluated on the fly.  kthin runs 1, 2, ... for every lane alike, so a
//   wavefront's loads stay whole rows; a lane whose bic turned negative leaves the loop and the
//   wavefront sweeps until its last lane has.
#define DG_CVM_U 8
#define DG_RF_BITS 4
#define DG_RF_DIGITS (1 << DG_RF_BITS)
#define DG_RF_U 8
static_assert(64 % DG_RF_BITS == 0, "the descent covers the 64 key bits in whole digits");

struct dg_starts {
  int64_t s[MMB_HEIDEL_MAX_STARTS];
};

template <int NS>
__global__ __launch_bounds__(DG_THREADS) void dg_cvm_kernel(int P, int K, int64_t n, int nstarts, dg_starts st,
                                                           const double* __restrict__ draws,
                                                           double* __restrict__ out) {
  const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int j = (int)blockIdx.y;
  if (k >= K) return;
  constexpr int U = DG_CVM_U;
  const size_t stride = (size_t)P * K;
  const double* p = draws + (size_t)j * K + k;
  const int64_t s0 = st.s[0];
  const double x0 = p[(size_t)s0 * stride];
  double mean[NS], B[NS], Q[NS];
#pragma unroll
  for (int q = 0; q < NS; ++q) mean[q] = B[q] = Q[q] = 0.0;
  // sweep 1: mean[] holds the suffix sums of x - x0 until the division below
  for (int q = 0; q < nstarts; ++q) {
    const int64_t a = st.s[q], b = q + 1 < nstarts ? st.s[q + 1] : n;
    double s = 0.0;
    for (int64_t t = a; t < b; t += 2 * U) {
      double xs[2 * U];
#pragma unroll
      for (int u = 0; u < 2 * U; ++u) xs[u] = dg_ld(p, stride, t + u, b);
#pragma unroll
      for (int u = 0; u < 2 * U; ++u) s += t + u < b ? xs[u] - x0 : 0.0;
    }
#pragma unroll
    for (int r = 0; r < NS; ++r) mean[r] += r <= q ? s : 0.0;
  }
#pragma unroll
  for (int q = 0; q < NS; ++q) mean[q] = q < nstarts ? x0 + mean[q] / (double)(n - st.s[q]) : 0.0;
  // sweep 2: a start past the current row (and a padded one, s = n) has B = 0 and adds nothing
  for (int64_t t = s0; t < n; t += U) {
    double xs[U];
#pragma unroll
    for (int u = 0; u < U; ++u) xs[u] = dg_ld(p, stride, t + u, n);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t r = t + u;
      const bool in = r < n;
#pragma unroll
      for (int q = 0; q < NS; ++q) {
        B[q] += in && r >= st.s[q] ? xs[u] - mean[q] : 0.0;
        Q[q] = fma(in ? B[q] : 0.0, B[q], Q[q]);
      }
    }
  }
  double* o = out + ((size_t)k * P + j) * nstarts * 2;
#pragma unroll
  for (int q = 0; q < NS; ++q)
    if (q < nstarts) {
      const double m = (double)(n - st.s[q]);
      o[2 * q] = mean[q];
      o[2 * q + 1] = Q[q] / (m * m);
    }
}

template <int ETYPE>
__global__ __launch_bounds__(DG_THREADS) void dg_mcse_from_kernel(int P, int K, const int64_t* __restrict__ i0s,
                                                                 int64_t i1, int64_t bs,
                                                                 const double* __restrict__ draws,
                                                                 double* __restrict__ out) {
  const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int j = (int)blockIdx.y;
  if (k >= K) return;
  const size_t stride = (size_t)P * K;
  const double* p = draws + (size_t)j * K + k;
  const int64_t i0 = i0s[(size_t)k * P + j];
  double* o = out + ((size_t)k * P + j) * MMB_MCSE_FIELDS;
  const double mean = dg_mean(p, stride, i0, i1);
  o[0] = mean;
  if (ETYPE == MMB_MCSE_BM) dg_bm(p, stride, i0, i1, bs, mean, o);
  else dg_iseq<ETYPE>(p, stride, i0, i1, mean, o);
}

// rlo: 0-based rank of the lower order statistic; interp: the quantile index is not an integer,
// the upper one has rank rlo + 1 and weight h.  n < 2^31 (32-bit counters).
__global__ __launch_bounds__(DG_THREADS) void dg_raftery_kernel(int P, int K, int64_t n, uint32_t rlo, int interp,
                                                               double h, const double* __restrict__ draws,
                                                               double* __restrict__ out) {
  const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int j = (int)blockIdx.y;
  if (k >= K) return;
  constexpr int U = DG_RF_U, ND = DG_RF_DIGITS;
  const size_t stride = (size_t)P * K;
  const double* p = draws + (size_t)j * K + k;
  // ---- select: after the sweep at shift sh the key bits sh .. 63 of the rank-rlo key are known
  uint64_t akey = 0ull;
  uint32_t rem = rlo;
  for (int sh = 64 - DG_RF_BITS; sh >= 0; sh -= DG_RF_BITS) {
    const uint64_t himask = sh == 64 - DG_RF_BITS ? 0ull : ~0ull << (sh + DG_RF_BITS);
    uint32_t cum[ND - 1];                        // cum[d] = keys under the prefix with digit <= d
#pragma unroll
    for (int d = 0; d < ND - 1; ++d) cum[d] = 0u;
    for (int64_t t = 0; t < n; t += U) {
      double xs[U];
#pragma unroll
      for (int u = 0; u < U; ++u) xs[u] = dg_ld(p, stride, t + u, n);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint64_t key = os_key(xs[u]);
        const bool ok = t + u < n && ((key ^ akey) & himask) == 0ull;
        const uint32_t dg = ok ? (uint32_t)(key >> sh) & (uint32_t)(ND - 1) : (uint32_t)ND;
#pragma unroll
        for (int d = 0; d < ND - 1; ++d) cum[d] += dg <= (uint32_t)d ? 1u : 0u;
      }
    }
    // the digit of the rank-rem key: the smallest one whose cumulative count exceeds rem
    uint32_t dsel = ND - 1, below = cum[ND - 2];
#pragma unroll
    for (int d = ND - 2; d >= 0; --d)
      if (cum[d] > rem) {
        dsel = (uint32_t)d;
        below = d > 0 ? cum[(d + ND - 2) % (ND - 1)] : 0u;   // cum[d - 1]
      }
    rem -= below;
    akey |= (uint64_t)dsel << sh;
  }
  const double a = os_unkey(akey);
  double thr = a;
  if (interp) {
    // the rank rlo + 1 statistic: a again when enough keys are <= a, else the smallest key above
    uint32_t cle = 0u;
    uint64_t nxt = ~0ull;
    for (int64_t t = 0; t < n; t += U) {
      double xs[U];
#pragma unroll
      for (int u = 0; u < U; ++u) xs[u] = dg_ld(p, stride, t + u, n);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint64_t key = os_key(xs[u]);
        const bool in = t + u < n;
        cle += in && key <= akey ? 1u : 0u;
        nxt = in && key > akey && key < nxt ? key : nxt;
      }
    }
    const double b = cle >= rlo + 2u ? a : os_unkey(nxt);
    const double wa = (1.0 - h) * a, wb = h * b;   // a multiply and an add each: the host formula's bits
    thr = wa + wb;
  }
  // ---- thinning loop (rafterydiag.jl:17-33)
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  double kthin = nan, bic = nan, c00 = 0.0, c10 = 0.0, c01 = 0.0, c11 = 0.0;
  int64_t ntest = n;
  for (int64_t kt = 1;; ++kt) {
    ntest = (n - 1) / kt + 1;                     // length(dichot[1:kt:n])
    if (ntest < 3) break;                         // reference: log(-1) throws
    uint32_t T[8];                                // T[a + 2b + 4c]: triples (a, b, c) = test[t .. t+2]
#pragma unroll
    for (int q = 0; q < 8; ++q) T[q] = 0u;
    uint32_t p1 = 0u, p2 = 0u;
    for (int64_t i = 0; i < ntest; i += U) {
      double xs[U];
#pragma unroll
      for (int u = 0; u < U; ++u) xs[u] = dg_ld(p, stride, (i + u) * kt, n);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool in = i + u < ntest;
        const uint32_t cur = xs[u] <= thr ? 1u : 0u;
        const uint32_t idx = in && i + u >= 2 ? p2 + 2u * p1 + 4u * cur : 8u;
#pragma unroll
        for (int q = 0; q < 8; ++q) T[q] += idx == (uint32_t)q ? 1u : 0u;
        p2 = in ? p1 : p2;
        p1 = in ? cur : p1;
      }
    }
    double g2 = 0.0;
#pragma unroll
    for (int ia = 0; ia < 2; ++ia)
#pragma unroll
      for (int ib = 0; ib < 2; ++ib)
#pragma unroll
        for (int ic = 0; ic < 2; ++ic) {
          const uint32_t tt = T[ia + 2 * ib + 4 * ic];
          if (tt > 0u) {
            const int64_t sa = (int64_t)T[2 * ib + 4 * ic] + T[1 + 2 * ib + 4 * ic];
            const int64_t sc = (int64_t)T[ia + 2 * ib] + T[ia + 2 * ib + 4];
            const int64_t sac = (int64_t)T[2 * ib] + T[1 + 2 * ib] + T[2 * ib + 4] + T[1 + 2 * ib + 4];
            const double fitted = (double)(sa * sc) / (double)sac;
            g2 += 2.0 * (double)tt * mmb_log((double)tt / fitted);
          }
        }
    bic = g2 - 2.0 * mmb_log((double)ntest - 2.0);
    if (!(bic >= 0.0)) {
      // tranfinal (rafterydiag.jl:34): the pairs are the triples' leading pairs and the last pair
      kthin = (double)kt;
      c00 = (double)(T[0] + T[4] + (p2 == 0u && p1 == 0u ? 1u : 0u));
      c10 = (double)(T[1] + T[5] + (p2 == 1u && p1 == 0u ? 1u : 0u));
      c01 = (double)(T[2] + T[6] + (p2 == 0u && p1 == 1u ? 1u : 0u));
      c11 = (double)(T[3] + T[7] + (p2 == 1u && p1 == 1u ? 1u : 0u));
      break;
    }
    bic = nan;
  }
  double* o = out + ((size_t)k * P + j) * MMB_RAFTERY_FIELDS;
  o[0] = thr;
  o[1] = kthin;
  o[2] = (double)ntest;
  o[3] = c00;
  o[4] = c10;
  o[5] = c01;
  o[6] = c11;
  o[7] = bic;
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

// starts: nstarts strictly increasing values in [0, n)
hipError_t mmb_launch_chain_cvm(int P, int K, int64_t n, int nstarts, const int64_t* starts, const double* draws,
                                double* out, hipStream_t st) {
  if (nstarts < 1 || nstarts > MMB_HEIDEL_MAX_STARTS) return hipErrorInvalidValue;
  dg_starts S;
  for (int q = 0; q < MMB_HEIDEL_MAX_STARTS; ++q) {
    S.s[q] = q < nstarts ? starts[q] : n;
    if (q < nstarts && (S.s[q] < 0 || S.s[q] >= n || (q > 0 && S.s[q] <= S.s[q - 1]))) return hipErrorInvalidValue;
  }
  const dim3 grid((K + DG_THREADS - 1) / DG_THREADS, P), blk(DG_THREADS);
  if (nstarts <= 8) hipLaunchKernelGGL(dg_cvm_kernel<8>, grid, blk, 0, st, P, K, n, nstarts, S, draws, out);
  else hipLaunchKernelGGL(dg_cvm_kernel<MMB_HEIDEL_MAX_STARTS>, grid, blk, 0, st, P, K, n, nstarts, S, draws, out);
  return hipGetLastError();
}

// i0s: K x P window starts on the device, each checked by the caller against i1 and the method
hipError_t mmb_launch_chain_mcse_from(int P, int K, const int64_t* i0s, int64_t i1, int etype, int64_t bs,
                                      const double* draws, double* out, hipStream_t st) {
  const dim3 grid((K + DG_THREADS - 1) / DG_THREADS, P), blk(DG_THREADS);
  if (etype == MMB_MCSE_BM) {
    if (bs < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dg_mcse_from_kernel<MMB_MCSE_BM>, grid, blk, 0, st, P, K, i0s, i1, bs, draws, out);
  } else if (etype == MMB_MCSE_IMSE) {
    hipLaunchKernelGGL(dg_mcse_from_kernel<MMB_MCSE_IMSE>, grid, blk, 0, st, P, K, i0s, i1, bs, draws, out);
  } else if (etype == MMB_MCSE_IPSE) {
    hipLaunchKernelGGL(dg_mcse_from_kernel<MMB_MCSE_IPSE>, grid, blk, 0, st, P, K, i0s, i1, bs, draws, out);
  } else {
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t mmb_launch_chain_raftery(int P, int K, int64_t n, int64_t rlo, int interp, double h, const double* draws,
                                    double* out, hipStream_t st) {
  if (n < 3 || n > 0x7fffffffll || rlo < 0 || rlo + (interp ? 1 : 0) >= n) return hipErrorInvalidValue;
  const dim3 grid((K + DG_THREADS - 1) / DG_THREADS, P), blk(DG_THREADS);
  hipLaunchKernelGGL(dg_raftery_kernel, grid, blk, 0, st, P, K, n, (uint32_t)rlo, interp, h, draws, out);
  return hipGetLastError();
}
