"""Element log densities of the node IR's ten families at 50 digits (mpmath) -- the checker of
csrc/ir_math.h's mmb_ir_lp at and near the support boundaries.

Restated from the mathematics, like ir_math.h itself; arguments in mmb_ir_lp's order
(x, a, b) = (value, first parameter, second parameter) with the double inputs taken as exact:

    normal       N(a, b)                 -(z^2 + log 2pi)/2 - log b,  z = (x - a)/b
    mvnormal     N(a[], b^2 I)           -(k log 2pi)/2 - k log b - sum (x - a)^2 / (2 b^2)
    invgamma     InverseGamma(a, b)      a log b - lgamma(a) - (a + 1) log x - b/x
    gamma        Gamma(a, scale b)       -lgamma(a) - a log b + (a - 1) log x - x/b
    exponential  Exponential(scale a)    -log a - x/a
    uniform      Uniform(lo, hi)         -log(hi - lo)
    beta         Beta(a, b)              (a-1) log x + (b-1) log(1-x) - lgamma(a) - lgamma(b) + lgamma(a+b)
    binomial     x of Binomial(a, b)     lchoose(a, x) + xlogy(x, b) + xlog1py(a - x, -b)
    poisson      x of Poisson(a)         xlogy(x, a) - a - lgamma(x + 1)
    bernoulli    x of Bernoulli(a)       x ? log a : log(1 - a)

Rules.
  * logpdf_sub: insupport(d, x) ? logpdf(d, x[, transform]) : -Inf.  A NaN x is outside every
    support.  Supports: normal all reals (x = +-Inf: the formula's -Inf), invgamma / gamma /
    exponential 0 <= x <= Inf, uniform lo <= x <= hi, beta 0 <= x <= 1, binomial the integers
    0..a, poisson the integers >= 0, bernoulli {0, 1}.
  * xlogy(0, 0) = 0 and xlog1py(0, -1) = 0: the density's own value where a coefficient vanishes.
  * Limits at the boundaries (the density is a limit there):
      beta at 0: +Inf if a < 1, the finite (b-1) log 1 - lbeta(a, b) = -lbeta(1, b) = log b if
        a = 1, -Inf if a > 1; mirrored at 1 with b.
      gamma at 0: +Inf, -log b, -Inf for a below, equal to and above 1.
      invgamma at 0: -Inf (exp(-b/x) beats every power).
      invgamma / gamma / exponential at +Inf: -Inf.
      poisson with rate +Inf (a rate expression such as lam * t can overflow): -Inf for every count.
  * transform = True adds the log Jacobian of the family's link: log x (invgamma, gamma,
    exponential), log(x (1 - x)) (beta), log((x - lo)(hi - x)/(hi - lo)) (uniform), nothing for
    the others.  Where the Jacobian is log 0 (or, for the log link at x = Inf, where the density
    is -Inf) the value is -Inf if the density is finite or -Inf there, and NaN (Inf - Inf, as the
    reference's Distributions arithmetic gives it) if the density is +Inf: check(..., tr=True)
    takes that NaN as "anything not finite".

Every function returns (v, M): v an mpf (mp.inf, mp.ninf, mp.nan included) and M, a float, the
sum of the absolute values of the formula's terms, where an lgamma(z) counts as
|(z - 1/2) log z| + z -- the size of what a Stirling evaluation adds up.  A double evaluation of
the formula is expected within a small multiple of 2^-53 M of v, whatever cancels.
"""
import math

import mpmath as mp

mp.mp.dps = 50
INF, NINF, NAN = mp.inf, mp.ninf, mp.nan
LOG2PI = mp.log(2 * mp.pi)
FAMILIES = ("normal", "mvnormal", "invgamma", "gamma", "exponential", "uniform", "beta", "binomial", "poisson",
            "bernoulli")


def _m(x):
    return mp.mpf(float(x))


def lgamma_scale(z):
    """|(z - 1/2) log z| + z: the magnitude of Stirling's terms for lgamma(z), z > 0."""
    z = _m(z)
    return abs((z - mp.mpf(0.5)) * mp.log(z)) + z


def _lg(z, terms):
    terms.append(lgamma_scale(z))
    return mp.loggamma(z)


def xlogy(c, x, terms):
    """c log x with 0 log 0 = 0."""
    if c == 0:
        return mp.mpf(0)
    v = c * mp.log(x) if x != 0 else (NINF if c > 0 else INF)
    if mp.isfinite(v):
        terms.append(abs(v))
    return v


def _sum(vals, terms):
    s = mp.mpf(0)
    for v in vals:
        s = s + v                       # inf + -inf = nan in mpmath too
        if mp.isfinite(v):
            terms.append(abs(v))
    return s


def _done(v, jac, terms):
    """Add the log Jacobian by the module's rule."""
    if jac is not None:
        if jac == NINF or (jac == INF and v == NINF):
            v = NAN if v == INF else NINF
        else:
            v = v + jac
            terms.append(abs(jac))
    return v, float(sum(terms, mp.mpf(0)))


def _isint(x):
    return mp.isfinite(x) and x == mp.floor(x)


def logpdf(fam, x, a=None, b=None, tr=False, lo=None, hi=None):
    """(v, M) of one element; mvnormal takes sequences x, a and a scalar b."""
    T = []
    if fam == "mvnormal":
        xs, mus, sg = [_m(t) for t in x], [_m(t) for t in a], _m(b)
        if not all(mp.isfinite(t) for t in xs):
            return NINF, 0.0
        k = len(xs)
        ss = sum(((t - u) ** 2 for t, u in zip(xs, mus)), mp.mpf(0))
        return _done(_sum([-k * LOG2PI / 2, -k * mp.log(sg), -ss / (2 * sg * sg)], T), None, T)
    x = _m(x)
    a = None if a is None else _m(a)
    b = None if b is None else _m(b)
    if mp.isnan(x):
        return NINF, 0.0
    if fam == "normal":
        if mp.isinf(x):
            return NINF, 0.0
        z = (x - a) / b
        return _done(_sum([-z * z / 2, -LOG2PI / 2, -mp.log(b)], T), None, T)
    if fam in ("invgamma", "gamma", "exponential"):
        if x < 0:
            return NINF, 0.0
        jac = (NINF if x == 0 else INF if x == INF else mp.log(x)) if tr else None
        if x == INF:
            return _done(NINF, jac, T)
        if fam == "exponential":
            return _done(_sum([-mp.log(a), -x / a], T), jac, T)
        if fam == "invgamma":
            if x == 0:
                return _done(NINF, jac, T)
            return _done(_sum([a * mp.log(b), -_lg(a, T), -(a + 1) * mp.log(x), -b / x], T), jac, T)
        head = _sum([-_lg(a, T), -a * mp.log(b), -x / b], T)
        return _done(head + xlogy(a - 1, x, T), jac, T)
    if fam == "uniform":
        lo, hi = _m(lo), _m(hi)
        if not (lo <= x <= hi):
            return NINF, 0.0
        jac = None
        if tr:
            q = (x - lo) * (hi - x) / (hi - lo)
            jac = NINF if q == 0 else mp.log(q)
        return _done(_sum([-mp.log(hi - lo)], T), jac, T)
    if fam == "beta":
        if not (0 <= x <= 1):
            return NINF, 0.0
        jac = None
        if tr:
            q = x * (1 - x)
            jac = NINF if q == 0 else mp.log(q)
        head = _sum([-_lg(a, T), -_lg(b, T), _lg(a + b, T)], T)
        return _done(head + xlogy(a - 1, x, T) + xlogy(b - 1, 1 - x, T), jac, T)
    if fam == "binomial":           # x = k, a = n, b = p
        if not (0 <= b <= 1):
            return NAN, 0.0
        if not (_isint(x) and 0 <= x <= a):
            return NINF, 0.0
        ch = _sum([_lg(a + 1, T), -_lg(x + 1, T), -_lg(a - x + 1, T)], T)
        return _done(ch + xlogy(x, b, T) + xlogy(a - x, 1 - b, T), None, T)
    if fam == "poisson":            # x = k, a = lambda
        if not (a >= 0):
            return NAN, 0.0
        if not (_isint(x) and x >= 0) or a == INF:
            return NINF, 0.0
        return _done(xlogy(x, a, T) + _sum([-a, -_lg(x + 1, T)], T), None, T)
    if fam == "bernoulli":          # x in {0, 1}, a = p
        if not (0 <= a <= 1):
            return NAN, 0.0
        if x not in (0, 1):
            return NINF, 0.0
        return _done(xlogy(mp.mpf(1), a if x == 1 else 1 - a, T), None, T)
    raise ValueError(fam)


def total(parts):
    """(v, M) of a sum of element or node terms [(v, M), ...]."""
    v = mp.mpf(0)
    for t, _ in parts:
        v = v + t
    return v, float(sum(m for _, m in parts))


def klass(v):
    """'nan', '+inf', '-inf' or 'finite' of an mpf or a float."""
    v = float(v)
    if math.isnan(v):
        return "nan"
    if math.isinf(v):
        return "+inf" if v > 0 else "-inf"
    return "finite"


def check(got, want, M, rtol=1e-12, atol=1e-13, where="", tr=False):
    """The tests' assertion: the class of `got` (a double) is that of `want`, exactly; a finite
    value lies within rtol M + atol.  One relaxation, for evaluations with the transform only
    (`tr`): a NaN reference there is the Inf - Inf of a +Inf density and a log 0 Jacobian (see the
    module text) and stands for "anything not finite".  Without `tr` a NaN reference (invalid
    parameters of a discrete family) asks for NaN."""
    kw = klass(want)
    if kw == "nan" and tr:
        assert not math.isfinite(got), (where, got, "want: not finite")
        return 0.0
    assert klass(got) == kw, (where, got, float(want))
    if kw != "finite":
        return 0.0
    err = float(abs(mp.mpf(float(got)) - want))
    assert err <= rtol * M + atol, (where, got, float(want), err, M)
    return err


# ---- the edge grid (tests/test_ir.py on the oracle's element layer, tests/test_gpu_ir_families.py on the device)
TINY = 5e-324                       # the smallest subnormal
ONE_M = 1.0 - 2.0 ** -53            # the largest double below 1
SHAPES = (1e-3, 0.5, 1.0, 2.0, 1e4)
PROBS = (0.0, TINY, 1e-300, 1e-8, 0.5, ONE_M, 1.0)
RATES = (0.0, TINY, 1e-300, 1e-8, 1.0, 1e300, 1e308)   # 2.5 * 1e308 overflows to Inf
_POS_X = (0.0, TINY, 1e-300, 1e-8, 1.0, 1e300, math.inf, -TINY, math.nan)
UNIFORM_LO, UNIFORM_HI = 0.5, 4.0   # the zoo's a ~ Uniform(0.5, 4): bounds are constants of the lowering


def edge_grid(fam):
    """[(x, a, b)] of a continuous family: every shape pair x (both support boundaries, the doubles
    just outside them, subnormal / tiny / interior / huge values as the support allows, NaN)."""
    if fam == "beta":
        xs = (0.0, TINY, 1e-300, 1e-8, 0.5, ONE_M, 1.0, -TINY, math.nextafter(1.0, 2.0), math.nan)
        return [(x, a, b) for a in SHAPES for b in SHAPES for x in xs]
    if fam in ("gamma", "invgamma"):
        return [(x, a, b) for a in SHAPES for b in SHAPES for x in _POS_X]
    if fam == "exponential":
        return [(x, a, None) for a in SHAPES for x in _POS_X]
    if fam == "normal":
        xs = (0.0, TINY, 1e-300, -1e-8, 1e300, -1e300, math.inf, -math.inf, math.nan)
        return [(x, a, b) for a in (0.0, -3.0) for b in SHAPES for x in xs]
    if fam == "uniform":
        lo, hi = UNIFORM_LO, UNIFORM_HI
        return [(x, None, None) for x in (lo, hi, math.nextafter(lo, -math.inf), math.nextafter(hi, math.inf), 1.0,
                                          math.nextafter(lo, math.inf), math.nextafter(hi, -math.inf), math.nan)]
    raise ValueError(fam)
