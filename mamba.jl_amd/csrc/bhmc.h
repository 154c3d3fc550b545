/*
 * bhmc.h — the per-element arithmetic of binary Hamiltonian Monte Carlo (src/samplers/bhmc.jl:50-122)
 * and the elementary functions it needs beyond mmb_math.h: atan2, and sin / cos of a plain angle in
 * [0, pi].  Plain C like mmb_math.h and symdist.h: the kernels (samplers.h bhmc) and a host C compiler
 * compile the same text, and tests/test_bhmc.py drives these functions from the host.
 *
 * Every operation is a comparison, an integer operation, one correctly rounded IEEE operation or an
 * explicit fma, so host and device return the same bits; build with -ffp-contract=off.
 *
 *   mmb_atan, mmb_atan2   fdlibm s_atan.c / e_atan2.c restated (as mmb_log / mmb_exp restate fdlibm):
 *                         signed zeros, infinities, NaN and all quadrants as there; < 1 ulp
 *   mmb_sincos            0 <= x <= pi: k = nearest multiple of pi/2 (0, 1 or 2), r = x - k pi/2 by a
 *                         Cody-Waite reduction with the split pi/2 = PIO2_1 + PIO2_1T (PIO2_1 holds 33
 *                         bits, so k PIO2_1 is exact), then fdlibm's kernels mmb_ksin / mmb_kcos on
 *                         |r| <= pi/4 and the quadrant's signs
 *   mmb_bhmc_walltime     time until the element reaches its wall: phi = atan2(position, velocity),
 *                         phi > 0 ? pi - phi : -phi (bhmc.jl:63-68); a NaN stays a NaN
 *   mmb_bhmc_guard        the last-hit guard (bhmc.jl:73-77): +Inf within 1e4 eps of 0 or of 2 pi
 *   mmb_bhmc_move         rotation by the angle whose sine and cosine are s and c (bhmc.jl:96-97)
 *   mmb_bhmc_bounce       the wall update of the element that hit (bhmc.jl:108-116)
 */
#ifndef MMB_BHMC_H
#define MMB_BHMC_H

#include "mmb_math.h"

#define MMB_BHMC_PI 3.14159265358979311600e+00      /* Float64(pi), the reference's `pi` in Float64 arithmetic */
#define MMB_BHMC_NEARZERO 2.220446049250313e-12    /* 1e4 * eps() (bhmc.jl:53) */

/* ------------------------------------------------------------------ atan (fdlibm s_atan.c) */
MMB_HD double mmb_atan(double x) {
  const double aT0 = 3.33333333333329318027e-01, aT1 = -1.99999999998764832476e-01,
               aT2 = 1.42857142725034663711e-01, aT3 = -1.11111104054623557880e-01,
               aT4 = 9.09088713343650656196e-02, aT5 = -7.69187620504482999495e-02,
               aT6 = 6.66107313738753120669e-02, aT7 = -5.83357013379057348645e-02,
               aT8 = 4.97687799461593236017e-02, aT9 = -3.65315727442169155270e-02,
               aT10 = 1.62858201153657823623e-02;
  const uint64_t u = mmb_d2u(x);
  const int32_t hx = (int32_t)(u >> 32);
  const int32_t ix = hx & 0x7fffffff;
  double hi = 0.0, lo = 0.0;
  int id;
  if (ix >= 0x44100000) { /* |x| >= 2^66 */
    if (ix > 0x7ff00000 || (ix == 0x7ff00000 && (uint32_t)u != 0u)) return x + x; /* NaN */
    const double r = 1.57079632679489655800e+00 + 6.12323399573676603587e-17;
    return hx > 0 ? r : -r;
  }
  if (ix < 0x3fdc0000) { /* |x| < 0.4375 */
    if (ix < 0x3e200000) return x; /* |x| < 2^-29 */
    id = -1;
  } else {
    x = fabs(x);
    if (ix < 0x3ff30000) {   /* |x| < 1.1875 */
      if (ix < 0x3fe60000) { /* 7/16 <= |x| < 11/16 */
        id = 0;
        hi = 4.63647609000806093515e-01;
        lo = 2.26987774529616870924e-17;
        x = (2.0 * x - 1.0) / (2.0 + x);
      } else { /* 11/16 <= |x| < 19/16 */
        id = 1;
        hi = 7.85398163397448278999e-01;
        lo = 3.06161699786838301793e-17;
        x = (x - 1.0) / (x + 1.0);
      }
    } else {
      if (ix < 0x40038000) { /* |x| < 2.4375 */
        id = 2;
        hi = 9.82793723247329054082e-01;
        lo = 1.39033110312309984516e-17;
        x = (x - 1.5) / (1.0 + 1.5 * x);
      } else { /* 2.4375 <= |x| < 2^66 */
        id = 3;
        hi = 1.57079632679489655800e+00;
        lo = 6.12323399573676603587e-17;
        x = -1.0 / x;
      }
    }
  }
  double z = x * x;
  const double w = z * z;
  const double s1 = z * (aT0 + w * (aT2 + w * (aT4 + w * (aT6 + w * (aT8 + w * aT10)))));
  const double s2 = w * (aT1 + w * (aT3 + w * (aT5 + w * (aT7 + w * aT9))));
  if (id < 0) return x - x * (s1 + s2);
  z = hi - ((x * (s1 + s2) - lo) - x);
  return hx < 0 ? -z : z;
}

/* ------------------------------------------------------------------ atan2 (fdlibm e_atan2.c) */
MMB_HD double mmb_atan2(double y, double x) {
  const double tiny = 1.0e-300, pi_o_4 = 7.8539816339744827900e-01, pi_o_2 = 1.5707963267948965580e+00,
               pi = 3.1415926535897931160e+00, pi_lo = 1.2246467991473531772e-16;
  const uint64_t ux = mmb_d2u(x), uy = mmb_d2u(y);
  const int32_t hx = (int32_t)(ux >> 32), hy = (int32_t)(uy >> 32);
  const int32_t ix = hx & 0x7fffffff, iy = hy & 0x7fffffff;
  const uint32_t lx = (uint32_t)ux, ly = (uint32_t)uy;
  if (ix > 0x7ff00000 || (ix == 0x7ff00000 && lx != 0u) || iy > 0x7ff00000 || (iy == 0x7ff00000 && ly != 0u))
    return x + y; /* x or y is NaN */
  if (hx == 0x3ff00000 && lx == 0u) return mmb_atan(y); /* x = 1.0 */
  const int m = (int)((((uint32_t)hy >> 31) & 1u) | (((uint32_t)hx >> 30) & 2u)); /* 2 sign(x) + sign(y) */
  if (((uint32_t)iy | ly) == 0u) { /* y = 0 */
    switch (m) {
      case 0:
      case 1: return y;           /* atan(+-0, +anything) = +-0 */
      case 2: return pi + tiny;   /* atan(+0, -anything) = pi */
      default: return -pi - tiny; /* atan(-0, -anything) = -pi */
    }
  }
  if (((uint32_t)ix | lx) == 0u) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny; /* x = 0 */
  if (ix == 0x7ff00000) { /* x is INF */
    if (iy == 0x7ff00000) {
      switch (m) {
        case 0: return pi_o_4 + tiny;        /* atan(+INF, +INF) */
        case 1: return -pi_o_4 - tiny;       /* atan(-INF, +INF) */
        case 2: return 3.0 * pi_o_4 + tiny;  /* atan(+INF, -INF) */
        default: return -3.0 * pi_o_4 - tiny; /* atan(-INF, -INF) */
      }
    } else {
      switch (m) {
        case 0: return 0.0;         /* atan(+..., +INF) */
        case 1: return -0.0;        /* atan(-..., +INF) */
        case 2: return pi + tiny;   /* atan(+..., -INF) */
        default: return -pi - tiny; /* atan(-..., -INF) */
      }
    }
  }
  if (iy == 0x7ff00000) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny; /* y is INF */
  const int32_t k = (iy - ix) >> 20;
  double z;
  if (k > 60) z = pi_o_2 + 0.5 * pi_lo;   /* |y / x| > 2^60 */
  else if (hx < 0 && k < -60) z = 0.0;    /* |y| / x < -2^60 */
  else z = mmb_atan(fabs(y / x));         /* safe to do y / x */
  switch (m) {
    case 0: return z;                 /* atan(+, +) */
    case 1: return -z;                /* atan(-, +) */
    case 2: return pi - (z - pi_lo);  /* atan(+, -) */
    default: return (z - pi_lo) - pi; /* atan(-, -) */
  }
}

/* ------------------------------------------------------------------ sin and cos of x, 0 <= x <= pi */
MMB_HD void mmb_sincos(double x, double* s, double* c) {
  const double invpio2 = 6.36619772367581382433e-01, /* 53 bits of 2 / pi */
               pio2_1 = 1.57079632673412561417e+00,  /* first 33 bits of pi / 2 */
               pio2_1t = 6.07710050650619224932e-11; /* pi / 2 - pio2_1 */
  const double kd = rint(x * invpio2); /* 0, 1 or 2 */
  double r = fma(-kd, pio2_1, x);      /* k pio2_1 is exact */
  r = fma(-kd, pio2_1t, r);
  const double sk = mmb_ksin(r), ck = mmb_kcos(r);
  switch ((int)kd & 3) {
    case 0: *s = sk; *c = ck; break;
    case 1: *s = ck; *c = -sk; break;
    case 2: *s = -sk; *c = -ck; break;
    default: *s = -ck; *c = sk; break;
  }
}

/* ------------------------------------------------------------------ the per-element steps of bhmc.jl */
MMB_HD double mmb_bhmc_walltime(double velocity, double position) {
  const double phi = mmb_atan2(position, velocity);
  return phi > 0.0 ? MMB_BHMC_PI - phi : -phi;
}

MMB_HD double mmb_bhmc_guard(double walltime) {
  return (fabs(walltime) < MMB_BHMC_NEARZERO || fabs(walltime - 2.0 * MMB_BHMC_PI) < MMB_BHMC_NEARZERO)
             ? __builtin_inf()
             : walltime;
}

/* a = velocity, b = position; a1, b1 the moved velocity and position */
MMB_HD void mmb_bhmc_move(double a, double b, double s, double c, double* a1, double* b1) {
  *a1 = a * c - b * s;
  *b1 = a * s + b * c;
}

/* sign(x) as Julia's: -1, 0 (of x's sign), 1, NaN for NaN */
MMB_HD double mmb_bhmc_sign(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : x); }

/* dlogf = logf(S with the element 1) - logf(S with the element 0).  Returns the element's new velocity:
 * crossed (v2 > 0, *crossed = 1) at the speed the energy leaves, or reflected (a NaN v2 reflects). */
MMB_HD double mmb_bhmc_bounce(double velocity, double dlogf, int* crossed) {
  const double sg = mmb_bhmc_sign(velocity);
  const double v2 = velocity * velocity + sg * 2.0 * dlogf;
  if (v2 > 0.0) {
    *crossed = 1;
    return sqrt(v2) * sg;
  }
  *crossed = 0;
  return velocity * -1.0;
}

#endif /* MMB_BHMC_H */
