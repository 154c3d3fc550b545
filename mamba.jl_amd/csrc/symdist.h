/*
 * symdist.h — standard variates of the reference's SymDistributionTypes other than Normal
 * (src/distributions/extensions.jl:51-53), the proposals RWM may take (src/samplers/rwm.jl:49-71).
 * Plain C like mmb_math.h: the kernels (samplers.h rwm) and a host program compile the same text.
 *
 * Like Philox in place of MersenneTwister, these samplers are a statistically equivalent deviation
 * from rand(d).  Coordinate k of a block takes the uniforms u_j = uniform #(8k + j)
 * of the block's MMB_SUB_PROPOSAL substream of (seed, global chain, iteration, block):
 *   SymUniform(0, 1)         2 u0 - 1
 *   SymTriangularDist(0, 1)  u0 - u1
 *   Epanechnikov(0, 1)       2 m - 1, m the 2nd smallest of u0..u2
 *   Biweight(0, 1)           2 m - 1, m the 3rd smallest of u0..u4
 *   Triweight(0, 1)          2 m - 1, m the 4th smallest of u0..u6
 *   Cosine(0, 1)             2 w - 1, w the root of G(w) = w - sin(2 pi w) / (2 pi) = u0 on [0, 1]
 * Epanechnikov, Biweight and Triweight are 2 Beta(k, k) - 1 for k = 2, 3, 4, and an integer Beta(k, k)
 * is the k-th order statistic of 2k - 1 uniforms: exact, no rejection loop.  G is the cdf of
 * (z + 1) / 2 for z ~ Cosine(0, 1); it is inverted by exactly 53 bisection steps from [0, 1].
 * Every operation is a comparison or one correctly rounded IEEE operation (mmb_sincos2pi is
 * mmb_math.h's), so host and device return the same bits; build with -ffp-contract=off.
 */
#ifndef MMB_SYMDIST_H
#define MMB_SYMDIST_H

#include "mmb_math.h"

/* `kind` below: mmb_rwm_proposal (include/mamba_hip.h) 1..6; 0 (Normal) draws from MMB_SUB_NORMAL */
#define MMB_SYM_UNIFORM 1
#define MMB_SYM_TRIANGULAR 2
#define MMB_SYM_EPANECHNIKOV 3
#define MMB_SYM_BIWEIGHT 4
#define MMB_SYM_TRIWEIGHT 5
#define MMB_SYM_COSINE 6

/* the (m + 1)-th smallest of u[0 .. 2m]: the element that m others precede (ties by index) */
MMB_HD double mmb_sym_median(const double* u, int m) {
  const int n = 2 * m + 1;
  double r = u[0];
  for (int i = 0; i < n; ++i) {
    int below = 0;
    for (int j = 0; j < n; ++j) below += (u[j] < u[i] || (u[j] == u[i] && j < i)) ? 1 : 0;
    r = below == m ? u[i] : r;
  }
  return r;
}

MMB_HD double mmb_sym_cosine(double u0) {
  double lo = 0.0, hi = 1.0;
#ifdef __clang__
#pragma unroll 1
#endif
  for (int i = 0; i < 53; ++i) {
    const double w = 0.5 * (lo + hi);
    double s, c;
    mmb_sincos2pi(w, &s, &c);
    if (w - s / MMB_TWOPI_HI < u0) lo = w;
    else hi = w;
  }
  return 2.0 * (0.5 * (lo + hi)) - 1.0;
}

/* uniforms #(8k) .. #(8k + 2m) of the substream, two per Philox block */
MMB_HD void mmb_sym_uniforms(const mmb_rng* s, uint32_t k, int m, double* u) {
  for (int q = 0; q <= m; ++q) {
    uint64_t a, b;
    mmb_rng_block(s, 4u * k + (uint32_t)q, &a, &b);
    u[2 * q] = mmb_u01(a);
    if (q < m) u[2 * q + 1] = mmb_u01(b);
  }
}

/* standard variate of coordinate k; s: the block's MMB_SUB_PROPOSAL stream */
MMB_HD double mmb_symdist(int kind, const mmb_rng* s, uint32_t k) {
  double u[7];
  switch (kind) {
    case MMB_SYM_UNIFORM:
      return 2.0 * mmb_uniform(s, 8u * k) - 1.0;
    case MMB_SYM_TRIANGULAR: {
      uint64_t a, b;
      mmb_rng_block(s, 4u * k, &a, &b);
      return mmb_u01(a) - mmb_u01(b);
    }
    case MMB_SYM_EPANECHNIKOV:
      mmb_sym_uniforms(s, k, 1, u);
      return 2.0 * mmb_sym_median(u, 1) - 1.0;
    case MMB_SYM_BIWEIGHT:
      mmb_sym_uniforms(s, k, 2, u);
      return 2.0 * mmb_sym_median(u, 2) - 1.0;
    case MMB_SYM_TRIWEIGHT:
      mmb_sym_uniforms(s, k, 3, u);
      return 2.0 * mmb_sym_median(u, 3) - 1.0;
    case MMB_SYM_COSINE:
      return mmb_sym_cosine(mmb_uniform(s, 8u * k));
    default:
      return __builtin_nan("");
  }
}

#endif /* MMB_SYMDIST_H */
