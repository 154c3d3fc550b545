/*
 * abc.h — the kernel densities of the ABC update (src/samplers/abc.jl:33: pdf(kernel(0.0, epsilon), d)) and its
 * summary codes, host and device.  Plain C like mmb_math.h: samplers.h abc and a host program compile the same text.
 *
 * kernel(0, eps) is Normal or a SymDistributionType (src/distributions/extensions.jl:51-53) with location 0 and
 * scale eps, evaluated at the distance d >= 0; u = d / eps:
 *   Normal             exp(-u^2 / 2) / (eps sqrt(2 pi))
 *   SymUniform         1 / (2 eps)                  for u <= 1, inclusive: with decay > 0 the tolerance
 *                                                   becomes a distance, and that draw has to weigh in
 *   SymTriangularDist  (1 - u) / eps
 *   Epanechnikov       0.75 (1 - u^2) / eps
 *   Biweight           (15 / 16) (1 - u^2)^2 / eps
 *   Triweight          (35 / 32) (1 - u^2)^3 / eps
 *   Cosine             (1 + cos(pi u)) / (2 eps)
 * Every kernel but Normal is 0 for u > 1.  A NaN distance or tolerance gives NaN (Normal, and the others
 * through u <= 1 being false: 0).  Every operation is one correctly rounded IEEE operation or mmb_math.h's
 * exp / sincos2pi, so host and device return the same bits; build with -ffp-contract=off.
 */
#ifndef MMB_ABC_H
#define MMB_ABC_H

#include "mamba_hip.h"
#include "mmb_math.h"
#include "symdist.h"
#include "predict_math.h"

#define MMB_ABC_SQRT2PI 2.50662827463100050242e+00

MMB_HD double mmb_abc_kernel_pdf(int kind, double eps, double d) {
  const double u = d / eps;
  if (kind == MMB_RWM_NORMAL) return mmb_exp(-(u * u) / 2.0) / (eps * MMB_ABC_SQRT2PI);
  if (!(u <= 1.0)) return 0.0;
  const double w = 1.0 - u * u;
  switch (kind) {
    case MMB_SYM_UNIFORM:
      return 1.0 / (2.0 * eps);
    case MMB_SYM_TRIANGULAR:
      return (1.0 - u) / eps;
    case MMB_SYM_EPANECHNIKOV:
      return 0.75 * w / eps;
    case MMB_SYM_BIWEIGHT:
      return 0.9375 * (w * w) / eps;
    case MMB_SYM_TRIWEIGHT:
      return 1.09375 * (w * w * w) / eps;
    case MMB_SYM_COSINE: {
      double s, c;
      mmb_sincos2pi(0.5 * u, &s, &c); /* cos(pi u) */
      return (1.0 + c) / (2.0 * eps);
    }
    default:
      return __builtin_nan("");
  }
}

/* pdf(Exponential(eps), x) = exp(-x / eps) / eps (randeps, abc.jl:74-76, 122-124) */
MMB_HD double mmb_abc_exp_pdf(double eps, double x) { return mmb_exp(-x / eps) / eps; }

/* the Philox block of simulation i (< MMB_ABC_MAX_NSIM) of draw k (0: the first update's simulation at the
 * current values; 1..maxdraw: the candidates) of sampler block b, slot j (< 16: the data node's position among
 * the block's data nodes; 16: randeps) -- on the substreams MMB_SUB_ABC_N / MMB_SUB_ABC_U (mmb_math.h) */
MMB_HD uint32_t mmb_abc_block(int b, int k, int i, int j) {
  return ((((uint32_t)b * (uint32_t)(MMB_ABC_MAX_DRAW + 1) + (uint32_t)k) * (uint32_t)MMB_ABC_MAX_NSIM + (uint32_t)i) *
          32u) + (uint32_t)j;
}

/* the data families: those mmb_pr_elem_on draws without a rejection loop */
MMB_HD int mmb_abc_data_family(int fam) {
  return fam == MMB_IR_NORMAL || fam == MMB_IR_ISONORMAL || fam == MMB_IR_BERNOULLI || fam == MMB_IR_BINOMIAL ||
         fam == MMB_IR_POISSON || fam == MMB_IR_EXPONENTIAL || fam == MMB_IR_UNIFORM;
}

#endif /* MMB_ABC_H */
