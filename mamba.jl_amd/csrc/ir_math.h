/*
 * ir_math.h — elementwise layer of the node IR, shared bit for bit by
 * the HIP kernels (ir.h) and the CPU oracle (oracle.c), like mmb_math.h: element log
 * densities of the Distributions 0.10 families (not vendored; formulas restated, DESIGN.md
 * §2), the transform rules of src/distributions/transformdistribution.jl:6-93, the unary
 * operators of the expression code (Mamba's invlogit/logit, src/utils.jl:64-68) and lgamma.
 * Pinned independently: element densities against scipy.stats and lgamma against libm
 * (tests/test_ir.py), and both against 50-digit references at and around every support
 * boundary (tests/ir_family_ref.py; on the device by tests/test_gpu_ir_families.py).
 * At a boundary a density is its limit there, never NaN: a NaN log density passes a Slice shrink
 * test !(lp < p0) as an improvement.
 */
#ifndef MMB_IR_MATH_H
#define MMB_IR_MATH_H
#include "mamba_hip.h"
#include "mmb_math.h"

/* lgamma(x) for x > 0: shift to z >= 10 by the product x(x+1)...(x+k-1), then Stirling's
 * series through z^-13 (truncation < 4e-17 at z = 10); ~1e-15 relative error. */
MMB_HD double mmb_lgamma(double x) {
  if (!(x > 0.0)) return x == 0.0 ? __builtin_inf() : __builtin_nan("");
  if (x > 1e300) return __builtin_inf();
  double z = x, p = 1.0;
  while (z < 10.0) {
    p = p * z;
    z = z + 1.0;
  }
  const double iz = 1.0 / z, iz2 = iz * iz;
  double s = 1.0 / 156.0;
  s = s * iz2 + (-691.0 / 360360.0);
  s = s * iz2 + (1.0 / 1188.0);
  s = s * iz2 + (-1.0 / 1680.0);
  s = s * iz2 + (1.0 / 1260.0);
  s = s * iz2 + (-1.0 / 360.0);
  s = s * iz2 + (1.0 / 12.0);
  const double half_log2pi = 0.91893853320467274178032973640561764;
  double r = (z - 0.5) * mmb_log(z) - z + half_log2pi + s * iz;
  if (p != 1.0) r = r - mmb_log(p);
  return r;
}

/* Mamba invlogit / logit (src/utils.jl:64-68) */
MMB_HD double mmb_invlogit(double x) { return 1.0 / (mmb_exp(-x) + 1.0); }
MMB_HD double mmb_logit(double x) { return mmb_log(x / (1.0 - x)); }

MMB_HD double mmb_ir_unary(int op, double a) {
  switch (op) {
    case MMB_IR_OP_NEG: return -a;
    case MMB_IR_OP_EXP: return mmb_exp(a);
    case MMB_IR_OP_LOG: return mmb_log(a);
    case MMB_IR_OP_SQRT: return sqrt(a);
    case MMB_IR_OP_INVLOGIT: return mmb_invlogit(a);
    case MMB_IR_OP_LOGIT: return mmb_logit(a);
    default: return a < 0.0 ? -a : a; /* MMB_IR_OP_ABS */
  }
}

/* link kind of a family (transformdistribution.jl): 0 identity (RealDistribution, 53-61),
 * 1 log (PositiveDistribution, 66-78), 2 logit (UnitDistribution, 83-93), 3 affine logit
 * (bounded TransformDistribution, 6-48) */
MMB_HD int mmb_ir_link_kind(int fam) {
  switch (fam) {
    case MMB_IR_INVGAMMA: case MMB_IR_GAMMA: case MMB_IR_EXPONENTIAL: return 1;
    case MMB_IR_BETA: return 2;
    case MMB_IR_UNIFORM: return 3;
    default: return 0;
  }
}
MMB_HD double mmb_ir_link(int kind, double x, double a, double b) {
  if (kind == 1) return mmb_log(x);
  if (kind == 2) return mmb_logit(x);
  if (kind == 3) return mmb_logit((x - a) / (b - a));
  return x;
}
MMB_HD double mmb_ir_invlink(int kind, double x, double a, double b) {
  if (kind == 1) return mmb_exp(x);
  if (kind == 2) return mmb_invlogit(x);
  if (kind == 3) return (b - a) * mmb_invlogit(x) + a;
  return x;
}

/* logpdf_sub(d, x, transform) of one element (distributionstruct.jl:138-140):
 * insupport(d, x) ? logpdf(d, x[, transform]) : -Inf.  (a, b) = the family's parameters in
 * Distributions order; ct = host-computed constant of a discrete observation (log binomial
 * coefficient, -lgamma(k+1)); [lo, hi] = Uniform bounds (constants). */
/* mmb_ir_lp's Normal with log(sigma) supplied (lb = mmb_log(b)): the generated kernels form it
   once for all the elements a lane evaluates when sigma does not depend on the element */
MMB_HD double mmb_ir_normal_lb(double x, double a, double b, double lb) {
  if (x != x) return -__builtin_inf();
  const double z = (x - a) / b;
  return -(z * z + MMB_LOG2PI) / 2.0 - lb;
}

/* c log x with xlogy's convention 0 log 0 = 0 (lx = mmb_log(x)): a Beta(1, b) or Gamma(1, theta)
 * density is finite at the boundary x = 0, where c * lx would be 0 * -Inf = NaN -- which the Slice
 * shrink test !(lp < p0) takes for a point inside the slice.  Every other (c, x) is the plain
 * product, so interior values keep their bits. */
MMB_HD double mmb_ir_xlogy(double c, double x, double lx) { return (c == 0.0 && x == 0.0) ? 0.0 : c * lx; }

/* insupport of the discrete families: x an integer in [lo, hi] (NaN: false) */
MMB_HD int mmb_ir_int_in(double x, double lo, double hi) { return lo <= x && x <= hi && x == floor(x); }

/* A sampled discrete node (updated by a DGS block, samplers.h dgs): its value is state, not a
 * host-checked observation, so insupport is tested here.  (lo, hi) = the node's support bounds;
 * Binomial's upper bound is the element's own n.  Categorical and DiscreteUniform test theirs in
 * mmb_ir_lp.  Observed nodes never come here: their densities keep their bits. */
MMB_HD int mmb_ir_discrete_in(int fam, double x, double n, double lo, double hi) {
  if (fam == MMB_IR_BINOMIAL) return mmb_ir_int_in(x, 0.0, n);
  if (fam == MMB_IR_BERNOULLI) return x == 0.0 || x == 1.0;
  return mmb_ir_int_in(x, lo, hi);
}

/* Offset into a node's constant table (mmb_ir_node.cterm) of element i with value x, -1 when x has no
 * entry: per element for observed nodes; lchoose(n_i, k) at i (hi + 1) + k for a sampled Binomial
 * node; p[x] at x - 1 for Categorical. */
MMB_HD int mmb_ir_cterm_index(int fam, int fixed, int i, double x, double lo, double hi) {
  if (fam == MMB_IR_CATEGORICAL) return mmb_ir_int_in(x, lo, hi) ? (int)x - 1 : -1;
  if (fam == MMB_IR_BINOMIAL && !fixed) return mmb_ir_int_in(x, 0.0, hi) ? i * ((int)hi + 1) + (int)x : -1;
  return i;
}

/* Dirichlet(alpha) (a node-level density, ir.h node_lp): element i contributes (alpha_i - 1) log x_i,
 * exactly 0 when alpha_i == 1 (xlogy: a flat coordinate is finite at x_i = 0).  The node is in its
 * support iff every x_i >= 0 and |sum x - 1| <= MMB_SIMPLEX_TOL (a NaN fails both); then
 * lp = sum_i t_i - lmnB, lmnB = sum lgamma(alpha_i) - lgamma(sum alpha_i) formed by the host. */
MMB_HD double mmb_ir_dirichlet_term(double alpha, double x) {
  const double c = alpha - 1.0;
  return c == 0.0 ? 0.0 : c * mmb_log(x);
}
MMB_HD double mmb_ir_dirichlet_lp(double st, double sx, int neg, double lmnb) {
  if (neg || !(fabs(sx - 1.0) <= MMB_SIMPLEX_TOL)) return -__builtin_inf();
  return st - lmnb;
}
/* Categorical(P), P a sampled Dirichlet node (cterm = MMB_IR_CAT_STATE(off)): the state offset of P */
MMB_HD int mmb_ir_cat_state(int fam, int cterm) { return fam == MMB_IR_CATEGORICAL && cterm <= -2 ? -2 - cterm : -1; }

MMB_HD double mmb_ir_lp(int fam, double x, double a, double b, double ct, int tr, double lo, double hi) {
  const double NINF = -__builtin_inf(), INF = __builtin_inf();
  switch (fam) {
    case MMB_IR_NORMAL: { /* normlogpdf(mu, sig, x) */
      if (x != x) return NINF;
      const double z = (x - a) / b;
      return -(z * z + MMB_LOG2PI) / 2.0 - mmb_log(b);
    }
    case MMB_IR_INVGAMMA: { /* a log b - lgamma(a) - (a + 1) log x - b / x */
      if (!(0.0 < x && x < INF)) return NINF; /* the density's limit at both ends of the support is 0 */
      const double lx = mmb_log(x);
      const double lp = a * mmb_log(b) - mmb_lgamma(a) - (a + 1.0) * lx - b / x;
      return tr ? lp + lx : lp;
    }
    case MMB_IR_GAMMA: { /* -lgamma(k) - k log theta + (k - 1) log x - x / theta */
      if (!(0.0 <= x && x < INF)) return NINF; /* x = Inf: the density's limit is 0 */
      if (tr && x == 0.0) return NINF;         /* x f(x) ~ x^k -> 0, also where f(0) = +Inf (k < 1) */
      const double lx = mmb_log(x);
      const double lp = -mmb_lgamma(a) - a * mmb_log(b) + mmb_ir_xlogy(a - 1.0, x, lx) - x / b;
      return tr ? lp + lx : lp;
    }
    case MMB_IR_EXPONENTIAL: { /* -log theta - x / theta */
      if (!(0.0 <= x && x < INF)) return NINF; /* x = Inf: the density's limit is 0 */
      const double lp = -mmb_log(a) - x / a;
      return tr ? lp + mmb_log(x) : lp;
    }
    case MMB_IR_UNIFORM: { /* -log(b - a); Jacobian log((x - a)(b - x)/(b - a)) */
      if (!(lo <= x && x <= hi)) return NINF;
      const double lp = -mmb_log(hi - lo);
      return tr ? lp + mmb_log((x - lo) * (hi - x) / (hi - lo)) : lp;
    }
    case MMB_IR_BETA: { /* (a-1) log x + (b-1) log(1-x) - lbeta(a, b); Jacobian log(x(1-x)) */
      if (!(0.0 <= x && x <= 1.0)) return NINF;
      if (tr && (x == 0.0 || x == 1.0)) return NINF; /* x(1-x) f(x) -> 0, also where f = +Inf (a or b < 1) */
      const double lb = mmb_lgamma(a) + mmb_lgamma(b) - mmb_lgamma(a + b);
      const double y = 1.0 - x;
      const double lp = mmb_ir_xlogy(a - 1.0, x, mmb_log(x)) + mmb_ir_xlogy(b - 1.0, y, mmb_log(y)) - lb;
      return tr ? lp + mmb_log(x * (1.0 - x)) : lp;
    }
    case MMB_IR_BINOMIAL: { /* lchoose(n, k) + xlogy(k, p) + xlog1py(n - k, -p) */
      const double t1 = x == 0.0 ? 0.0 : x * mmb_log(b);
      const double t2 = (a - x) == 0.0 ? 0.0 : (a - x) * mmb_log1p(-b);
      return ct + t1 + t2;
    }
    case MMB_IR_POISSON: { /* xlogy(k, lambda) - lambda - lgamma(k + 1) */
      if (a == INF) return NINF; /* the limit; k log(Inf) - Inf is NaN (a rate expression can overflow) */
      const double t1 = x == 0.0 ? 0.0 : x * mmb_log(a);
      return ct + t1 - a;
    }
    case MMB_IR_BERNOULLI: /* x ? log p : log(1 - p) */
      return x == 1.0 ? mmb_log(a) : mmb_log(1.0 - a);
    case MMB_IR_CATEGORICAL: /* log p[x], x in 1..K = lo..hi; ct = p[x] (looked up by the caller) */
      if (!mmb_ir_int_in(x, lo, hi)) return NINF;
      return mmb_log(ct);
    case MMB_IR_DISCRETEUNIFORM: /* -log(b - a + 1) on the integers a..b */
      if (!mmb_ir_int_in(x, lo, hi)) return NINF;
      return -mmb_log(hi - lo + 1.0);
    default:
      return 0.0; /* Logical nodes contribute 0 */
  }
}

#endif /* MMB_IR_MATH_H */
