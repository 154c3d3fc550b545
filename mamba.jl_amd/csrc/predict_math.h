/*
 * predict_math.h — one posterior predictive variate of a node element (predict.hip), host and device.
 *
 * predict(mc, nodekeys) (src/output/modelstats.jl:71-102) draws rand(m[key]) from Julia's global RNG
 * for every kept draw.  Here a predicted value is a pure function of (seed, global chain id,
 * iteration of the kept row, node id n, element e) on the Philox layout of mmb_math.h:
 *   node block     PB(n)    = 256 + n                (sampler blocks are < 8)
 *   element block  GB(n, e) = (n + 1) * 65536 + e    (gamma-based families; needs 2 len <= 65536 and
 *                                                     a tag that fits 32 bits: predict.hip validates)
 * Normal, IsoNormal   a + b z, z = normal #e of (PB, MMB_SUB_NORMAL)
 * Bernoulli           u < p ? 1 : 0, u = uniform #e of (PB, MMB_SUB_UNIFORM)
 * Exponential(theta)  -theta log1p(-u);  Uniform(lo, hi)  lo + (hi - lo) u
 * Binomial(n, p)      the trials in chunks of at most 512, chunk c with uniform #(c len + e):
 *                     sequential-search inversion on p' = min(p, 1 - p), mirrored when p > 1/2
 * Poisson(lambda)     m = max(1, ceil(lambda / 256)) pieces of lambda / m, piece c with uniform
 *                     #(c len + e): sequential-search inversion, at most 4096 steps; m > 64 -> NaN
 * Gamma(k, theta)     theta G(k);  InverseGamma(a, b)  b / G(a);  Beta(a, b)  G1 / (G1 + G2) with
 *                     G1 = G(a) on GB(n, e) and G2 = G(b) on GB(n, len + e); G = mmb_gamma_any on the
 *                     block's MMB_SUB_GAMMA_N / _U substreams, running indices from 0
 * A parameter that is not finite or lies outside the family's domain gives NaN and draws nothing, so
 * every loop ends: the Marsaglia-Tsang rejection loop is never entered with a non-finite shape, and
 * the two searches are bounded by their caps whatever u and the running cdf are.
 */
#ifndef MMB_PREDICT_MATH_H
#define MMB_PREDICT_MATH_H
#include "mamba_hip.h"
#include "mmb_math.h"

#define MMB_PR_BLOCK0 256u
#define MMB_PR_BINOM_CHUNK 512
#define MMB_PR_BINOM_NMAX 1048576.0 /* trials of one Binomial element (2048 chunks); more -> NaN */
#define MMB_PR_POIS_PIECE 256.0
#define MMB_PR_POIS_PIECES 64
#define MMB_PR_POIS_STEPS 4096

MMB_HD uint32_t mmb_pr_block(int n) { return MMB_PR_BLOCK0 + (uint32_t)n; }
MMB_HD uint32_t mmb_pr_gblock(int n, int e) { return ((uint32_t)n + 1u) * 65536u + (uint32_t)e; }
/* the gamma-based families' tags of node n fit 32 bits: ((n + 2) 65536) 16 <= 2^32, and 2 len <= 65536 */
MMB_HD int mmb_pr_gblock_ok(int n, int len) { return n >= 0 && n + 2 <= 4096 && len >= 1 && 2 * (int64_t)len <= 65536; }

MMB_HD double mmb_pr_binomial(double n, double p, const mmb_rng* su, uint32_t e, uint32_t len) {
  if (!(n >= 0.0 && n <= MMB_PR_BINOM_NMAX) || n != rint(n) || !(p >= 0.0 && p <= 1.0)) return __builtin_nan("");
  if (p == 0.0) return 0.0;
  if (p == 1.0) return n;
  const int flip = p > 0.5;
  const double pp = flip ? 1.0 - p : p;
  const double q = 1.0 - pp, s = pp / q;
  const double l1 = mmb_log1p(-pp);
  const int nt = (int)n;
  const int C = (nt + MMB_PR_BINOM_CHUNK - 1) / MMB_PR_BINOM_CHUNK;
  double tot = 0.0;
  for (int c = 0; c < C; ++c) {
    const int nc = c < C - 1 ? MMB_PR_BINOM_CHUNK : nt - MMB_PR_BINOM_CHUNK * (C - 1);
    const double u = mmb_uniform(su, (uint32_t)c * len + e);
    double r = mmb_exp((double)nc * l1);
    double cdf = r;
    int k = 0;
    while (u > cdf && k < nc) {
      ++k;
      r = r * (s * (double)(nc - k + 1) / (double)k);
      cdf = cdf + r;
    }
    tot = tot + (double)(flip ? nc - k : k);
  }
  return tot;
}

MMB_HD double mmb_pr_poisson(double lam, const mmb_rng* su, uint32_t e, uint32_t len) {
  if (!(lam >= 0.0) || !isfinite(lam)) return __builtin_nan("");
  const double md = ceil(lam / MMB_PR_POIS_PIECE);
  if (md > (double)MMB_PR_POIS_PIECES) return __builtin_nan("");
  const int m = md < 1.0 ? 1 : (int)md;
  const double lp = lam / (double)m;
  const double r0 = mmb_exp(-lp);
  double tot = 0.0;
  for (int c = 0; c < m; ++c) {
    const double u = mmb_uniform(su, (uint32_t)c * len + e);
    double r = r0, cdf = r0;
    int k = 0;
    while (u > cdf && k < MMB_PR_POIS_STEPS) {
      ++k;
      r = r * (lp / (double)k);
      cdf = cdf + r;
    }
    tot = tot + (double)k;
  }
  return tot;
}

/* G(a) on the element block gb; a finite and > 0 (the callers check) */
MMB_HD double mmb_pr_gamma(double a, uint64_t seed, uint32_t chain, uint32_t iter, uint32_t gb) {
  const mmb_rng sn = mmb_rng_make(seed, chain, iter, gb, MMB_SUB_GAMMA_N);
  const mmb_rng su = mmb_rng_make(seed, chain, iter, gb, MMB_SUB_GAMMA_U);
  uint32_t kn = 0, ku = 0;
  return mmb_gamma_any(a, &sn, &su, &kn, &ku);
}

/* element e of a node of family fam and length len with parameters (a, b) in Distributions order, for the
 * families that draw without a rejection loop: the normal of stream sn or the uniforms of stream su.  The
 * body of mmb_pr_elem below, and of the ABC update's simulated data (samplers.h abc) on streams of its own. */
MMB_HD double mmb_pr_elem_on(int fam, double a, double b, const mmb_rng* sn, const mmb_rng* su, int e, int len) {
  const double NAN_ = __builtin_nan("");
  switch (fam) {
    case MMB_IR_NORMAL:
    case MMB_IR_ISONORMAL:
      if (!isfinite(a) || !isfinite(b) || b < 0.0) return NAN_;
      return a + b * mmb_normal(sn, (uint32_t)e);
    case MMB_IR_BERNOULLI:
      if (!(a >= 0.0 && a <= 1.0)) return NAN_;
      return mmb_uniform(su, (uint32_t)e) < a ? 1.0 : 0.0;
    case MMB_IR_EXPONENTIAL:
      if (!isfinite(a) || !(a > 0.0)) return NAN_;
      return -a * mmb_log1p(-mmb_uniform(su, (uint32_t)e));
    case MMB_IR_UNIFORM:
      if (!isfinite(a) || !isfinite(b) || b < a) return NAN_;
      return a + (b - a) * mmb_uniform(su, (uint32_t)e);
    case MMB_IR_BINOMIAL:
      return mmb_pr_binomial(a, b, su, (uint32_t)e, (uint32_t)len);
    case MMB_IR_POISSON:
      return mmb_pr_poisson(a, su, (uint32_t)e, (uint32_t)len);
    default:
      return NAN_;
  }
}

/* element e of node n (family fam, length len) with parameters (a, b) in Distributions order */
MMB_HD double mmb_pr_elem(int fam, double a, double b, uint64_t seed, uint32_t chain, uint32_t iter, int n, int e,
                          int len) {
  const double NAN_ = __builtin_nan("");
  switch (fam) {
    case MMB_IR_NORMAL:
    case MMB_IR_ISONORMAL:
    case MMB_IR_BERNOULLI:
    case MMB_IR_EXPONENTIAL:
    case MMB_IR_UNIFORM:
    case MMB_IR_BINOMIAL:
    case MMB_IR_POISSON: {
      const mmb_rng sn = mmb_rng_make(seed, chain, iter, mmb_pr_block(n), MMB_SUB_NORMAL);
      const mmb_rng su = mmb_rng_make(seed, chain, iter, mmb_pr_block(n), MMB_SUB_UNIFORM);
      return mmb_pr_elem_on(fam, a, b, &sn, &su, e, len);
    }
    case MMB_IR_GAMMA:
    case MMB_IR_INVGAMMA:
    case MMB_IR_BETA: {
      if (!isfinite(a) || !isfinite(b) || !(a > 0.0) || !(b > 0.0)) return NAN_;
      const double g1 = mmb_pr_gamma(a, seed, chain, iter, mmb_pr_gblock(n, e));
      if (fam == MMB_IR_GAMMA) return b * g1;
      if (fam == MMB_IR_INVGAMMA) return b / g1;
      const double g2 = mmb_pr_gamma(b, seed, chain, iter, mmb_pr_gblock(n, len + e));
      return g1 / (g1 + g2);
    }
    default:
      return NAN_;
  }
}

#endif /* MMB_PREDICT_MATH_H */
