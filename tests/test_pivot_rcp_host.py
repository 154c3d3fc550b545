"""The seeded reciprocal of the optimistic factorization pass (device.h mmb_rcp_seeded), restated
on the host: from a seed r0 near 1 / s, one Newton step and the final correction,

    e = fma(-s, r, 1); r = fma(r, e, r); e = fma(-s, r, 1); result = fma(e, r, r),

must give 1.0 / s bit for bit wherever mmb_rcp_seeded_doubt is false for the pivot candidate x
with sqrt(x) = s (the pass sends the others to the checked pass, which divides).  The device's
seed is twice the square root's Goldschmidt half-reciprocal, good to a few 2^-52; here the seed
is RN(1 / s) displaced by 0, +-1, +-2, +-3 ulps, so the check does not depend on v_rsq_f64.

A small C program (host compiler, -ffp-contract=off, fma() from libm) runs s over
* 2^k - n ulps (all-ones and near-all-ones significands) and 2^k + n ulps, n <= 64, for every
  binade edge 2^k whose square is in the fast range [2^-700, 2^700];
* sqrt(x) for x = 2^e -+ n ulps, n <= 64, every e in [-700, 700];
* 10^7 random s (random significand, exponent uniform in [-350, 350)).
For each s the x that round to it are found by scanning RN(s^2) +- 4 ulps with the IEEE sqrt; a
mismatch counts as a violation unless the predicate holds for every one of them (no such x: always
a violation).  The predicate's size is counted as well: at most 2^-40 of the significands."""
import json
import os
import shutil
import subprocess

import pytest

SRC = r"""
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
static double u2d(uint64_t u) { double d; memcpy(&d, &u, 8); return d; }
static uint64_t d2u(double d) { uint64_t u; memcpy(&u, &d, 8); return u; }
static int fast_range(double x) { return x >= 0x1p-700 && x <= 0x1p700; }
/* device.h mmb_rcp_seeded_doubt */
static int doubt(double x) { return ((d2u(x) + 64ull) & 0xFFFFFFFFFFFFFull) <= 128ull; }
/* device.h mmb_rcp_seeded after r = h + h */
static double rcp_short(double s, double r) {
  double e = fma(-s, r, 1.0);
  r = fma(r, e, r);
  e = fma(-s, r, 1.0);
  return fma(e, r, r);
}
static long cases, mismatches, violations, covered, shown;
static void one(double s) {
  if (!(s > 0.0) || !fast_range(s * s)) return;
  /* every in-range x with sqrt(x) == s; clear = some such x passes the predicate, or there is none */
  const uint64_t x0 = d2u(s * s);
  int nx = 0, ndoubt = 0;
  for (int k = -4; k <= 4; ++k) {
    const double x = u2d(x0 + (int64_t)k);
    if (fast_range(x) && sqrt(x) == s) { ++nx; ndoubt += doubt(x); }
  }
  const int clear = nx == 0 || ndoubt < nx;
  const double ref = 1.0 / s;
  for (int dsp = -3; dsp <= 3; ++dsp) {
    const double r = rcp_short(s, u2d(d2u(ref) + (int64_t)dsp));
    ++cases;
    if (r != ref) {
      ++mismatches;
      if (clear) {
        ++violations;
        if (shown++ < 20) fprintf(stderr, "violation: s %a seed %+d ulps: %a != %a\n", s, dsp, r, ref);
      } else {
        ++covered;
      }
    }
  }
}
int main(void) {
  for (int k = -351; k <= 351; ++k)
    for (int n = -64; n <= 64; ++n) one(u2d(d2u(ldexp(1.0, k)) + (int64_t)n));
  for (int e = -700; e <= 700; ++e)
    for (int n = -64; n <= 64; ++n) one(sqrt(u2d(d2u(ldexp(1.0, e)) + (int64_t)n)));
  const long directed = cases;
  uint64_t z = 88172645463325252ull;
  long random_doubt = 0;
  for (long i = 0; i < 10000000; ++i) {
    z ^= z << 13; z ^= z >> 7; z ^= z << 17;
    const double m = u2d(0x3FF0000000000000ull | (z & 0xFFFFFFFFFFFFFull));
    const double s = ldexp(m, (int)((z >> 52) % 700u) - 350);
    random_doubt += doubt(s * s);
    one(s);
  }
  /* significands the predicate covers: only those near the two ends of a binade can be */
  long pred = 0;
  for (uint64_t m = 0; m < (1u << 13); ++m) {
    pred += doubt(u2d(0x3FF0000000000000ull | m));
    pred += doubt(u2d(0x3FF0000000000000ull | (0xFFFFFFFFFFFFFull - m)));
  }
  const int mid = doubt(1.5) || doubt(1.25) || doubt(3.0) || doubt(u2d(0x3FF0000000002000ull));
  printf("{\"cases\": %ld, \"directed_cases\": %ld, \"mismatches\": %ld, \"covered\": %ld, \"violations\": %ld, "
         "\"predicate_significands\": %ld, \"predicate_mid_hits\": %d, \"random_doubt\": %ld}\n",
         cases, directed, mismatches, covered, violations, pred, mid, random_doubt);
  return 0;
}
"""


@pytest.fixture(scope="module")
def result(tmp_path_factory):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no host C compiler")
    tmp = tmp_path_factory.mktemp("pivot_rcp")
    src, exe = os.path.join(tmp, "pivot_rcp.c"), os.path.join(tmp, "pivot_rcp")
    with open(src, "w") as f:
        f.write(SRC)
    subprocess.run([cc, "-O2", "-ffp-contract=off", src, "-o", exe, "-lm"], check=True)
    r = subprocess.run([exe], check=True, capture_output=True, text=True)
    print(r.stdout, r.stderr)
    return json.loads(r.stdout), r.stderr


def test_short_reciprocal_is_exact_outside_the_predicate(result):
    res, err = result
    assert res["directed_cases"] > 7 * 129 * 1400
    assert res["cases"] - res["directed_cases"] == 7 * 10 ** 7
    assert res["violations"] == 0, err
    # the predicate is not vacuous: the all-ones significands do come out wrong from an inexact seed
    assert res["covered"] == res["mismatches"] > 0


def test_predicate_covers_at_most_2_pow_minus_40(result):
    res, _ = result
    assert 0 < res["predicate_significands"] <= 2 ** 12   # of 2^52 significands
    assert res["predicate_mid_hits"] == 0
    assert res["random_doubt"] == 0
