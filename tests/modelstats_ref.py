"""Restatement of src/output/modelstats.jl in numpy + math.fsum / math.lgamma (no project code).

logpdf(mc, nodekeys) (modelstats.jl:30-68): for every kept draw, the model's nodes take the draw's
values and the log densities of the listed nodes are added in list order (modelstats.jl:63).
dic(mc) (modelstats.jl:3-12): Dhat = -2 logpdf at the column means (modelstats.jl:15-25),
D = -2 logpdf per draw, p = [mean(D) - Dhat, 0.5 var(D)], value = [Dhat + 2p, p].

A model description is a dict
    "cols":   node name -> monitored column indices of the n x p x K value array
    "lp":     node name -> f(vals) -> float, vals = {node name: 1-d array of the draw's values}
Element sums are math.fsum (exact), so a description is a reference, not a second implementation
of the device's summation order.
"""
import math

import numpy as np

LOG2PI = math.log(2.0 * math.pi)
NINF = float("-inf")


# ---- node log densities (Distributions' formulas; support -> -Inf) -------------------------
def normal_lp(x, mu, sig):
    if math.isnan(x):
        return NINF
    z = (x - mu) / sig
    return -0.5 * z * z - math.log(sig) - 0.5 * LOG2PI


def normal_vec_lp(x, mu, sig):
    """A vector node with a univariate Normal per element: the sum of the element terms."""
    x, mu, sig = np.broadcast_arrays(np.asarray(x, float), np.asarray(mu, float), np.asarray(sig, float))
    return math.fsum(normal_lp(float(a), float(b), float(c)) for a, b, c in zip(x, mu, sig))


def iso_normal_lp(x, mu, sig):
    """MvNormal(mu, sig) with covariance sig^2 I; insupport = every element finite."""
    x = np.asarray(x, float)
    mu = np.broadcast_to(np.asarray(mu, float), x.shape)
    if not np.all(np.isfinite(x)):
        return NINF
    k = x.size
    ss = math.fsum(float((a - b) * (a - b)) for a, b in zip(x, mu))
    return -0.5 * (k * LOG2PI + k * math.log(sig * sig) + ss / (sig * sig))


def invgamma_lp(x, a, b):
    if not 0.0 <= x <= math.inf:
        return NINF
    if x == 0.0:
        return NINF
    return a * math.log(b) - math.lgamma(a) - (a + 1.0) * math.log(x) - b / x


def binomial_lp(k, n, p):
    t1 = 0.0 if k == 0 else k * math.log(p)
    t2 = 0.0 if n - k == 0 else (n - k) * math.log1p(-p)
    return math.lgamma(n + 1.0) - math.lgamma(k + 1.0) - math.lgamma(n - k + 1.0) + t1 + t2


def binomial_vec_lp(k, n, p):
    return math.fsum(binomial_lp(float(a), float(b), float(c)) for a, b, c in zip(k, n, p))


def invlogit(x):
    return 1.0 / (np.exp(-np.asarray(x, float)) + 1.0)


# ---- logpdf / dic ---------------------------------------------------------------------------
def logpdf_point(x, desc, keys):
    """The listed nodes' summed log density at one point x (p values in column order)."""
    x = np.asarray(x, float)
    vals = {name: x[np.asarray(cols)] for name, cols in desc["cols"].items()}
    lp = 0.0
    for key in keys:
        lp = lp + desc["lp"][key](vals)
    return lp


def logpdf_draws(value, desc, keys):
    """n x K: logpdf(mc, nodekeys).value[:, 1, :]."""
    n, _, K = value.shape
    out = np.empty((n, K))
    for i in range(n):
        for k in range(K):
            out[i, k] = logpdf_point(value[i, :, k], desc, keys)
    return out


def dic(value, desc, keys):
    """(2 x 2 [[DIC_pD, pD], [DIC_pV, pV]], Dhat)."""
    n, p, K = value.shape
    means = np.array([math.fsum(value[:, j, :].ravel()) / (n * K) for j in range(p)])
    dhat = -2.0 * logpdf_point(means, desc, keys)
    D = -2.0 * logpdf_draws(value, desc, keys)
    pv = np.array([np.mean(D) - dhat, 0.5 * np.var(D, ddof=1)])
    return np.column_stack([dhat + 2.0 * pv, pv]), dhat


# ---- descriptions of the models the tests use -----------------------------------------------
LINE_X = np.array([1.0, 2, 3, 4, 5])
LINE_Y = np.array([1.0, 3, 3, 3, 5])


def line_desc():
    """doc/tutorial/line.jl:5-25, monitored beta[1], beta[2], s2."""
    return {"cols": {"beta": [0, 1], "s2": [2]},
            "lp": {"y": lambda v: iso_normal_lp(LINE_Y, v["beta"][0] + v["beta"][1] * LINE_X, math.sqrt(v["s2"][0])),
                   "beta": lambda v: iso_normal_lp(v["beta"], 0.0, math.sqrt(1000.0)),
                   "s2": lambda v: invgamma_lp(float(v["s2"][0]), 0.001, 0.001)}}


def seeds_desc(data):
    """doc/examples/seeds.jl:16-56 with b monitored: columns b[1..21], alpha0, alpha1, alpha2, alpha12, s2."""
    r, n = np.asarray(data["r"], float), np.asarray(data["n"], float)
    x1, x2 = np.asarray(data["x1"], float), np.asarray(data["x2"], float)

    def eta(v):
        return v["alpha0"][0] + v["alpha1"][0] * x1 + v["alpha2"][0] * x2 + v["alpha12"][0] * x1 * x2 + v["b"]

    cols = {"b": list(range(21)), "alpha0": [21], "alpha1": [22], "alpha2": [23], "alpha12": [24], "s2": [25]}
    lp = {"r": lambda v: binomial_vec_lp(r, n, invlogit(eta(v))),
          "b": lambda v: normal_vec_lp(v["b"], 0.0, math.sqrt(v["s2"][0])),
          "s2": lambda v: invgamma_lp(float(v["s2"][0]), 0.001, 0.001)}
    for a in ("alpha0", "alpha1", "alpha2", "alpha12"):
        lp[a] = (lambda nm: lambda v: normal_lp(float(v[nm][0]), 0.0, 1000.0))(a)
    return {"cols": cols, "lp": lp}


def rats_desc(y, rat, Xm):
    """doc/examples/rats.jl:48-97 with every sampled node and the Logical alpha0 monitored: columns
    alpha[1..30], alpha0, mu_alpha, s2_alpha, beta[1..30], mu_beta, s2_beta, s2_c (`rat` 0-based).
    The alpha0 column is not read: no Stochastic node depends on it."""
    y, rat, Xm = np.asarray(y, float), np.asarray(rat, int), np.asarray(Xm, float)
    cols = {"alpha": list(range(30)), "mu_alpha": [31], "s2_alpha": [32], "beta": list(range(33, 63)),
            "mu_beta": [63], "s2_beta": [64], "s2_c": [65]}
    lp = {"y": lambda v: iso_normal_lp(y, v["alpha"][rat] + v["beta"][rat] * Xm, math.sqrt(v["s2_c"][0])),
          "alpha": lambda v: normal_vec_lp(v["alpha"], v["mu_alpha"][0], math.sqrt(v["s2_alpha"][0])),
          "beta": lambda v: normal_vec_lp(v["beta"], v["mu_beta"][0], math.sqrt(v["s2_beta"][0])),
          "mu_alpha": lambda v: normal_lp(float(v["mu_alpha"][0]), 0.0, 1000.0),
          "mu_beta": lambda v: normal_lp(float(v["mu_beta"][0]), 0.0, 1000.0)}
    for a in ("s2_alpha", "s2_beta", "s2_c"):
        lp[a] = (lambda nm: lambda v: invgamma_lp(float(v[nm][0]), 0.001, 0.001))(a)
    return {"cols": cols, "lp": lp}


def bigvec_desc(z, m):
    """theta[1..m] ~ Normal(0, 2) elementwise, z[1..m] ~ Normal(theta, 0.5) observed."""
    z = np.asarray(z, float)
    return {"cols": {"theta": list(range(m))},
            "lp": {"z": lambda v: normal_vec_lp(z, v["theta"], 0.5),
                   "theta": lambda v: normal_vec_lp(v["theta"], 0.0, 2.0)}}


class FakeEngine:
    """The three engine entry points dic_sharded uses, by the restatement, on a host array."""

    def __init__(self, value, desc, names_by_id):
        self.value = np.asarray(value, float)
        self.desc, self.names = desc, names_by_id
        self.K, self.pmon = self.value.shape[2], self.value.shape[1]

    def num_kept(self):
        return self.value.shape[0]

    def chain_summary(self, shift, batch_size=100, chain_base=0):
        out = np.zeros((self.K, self.pmon, 10))
        for k in range(self.K):
            for j in range(self.pmon):
                out[k, j, 0] = math.fsum(self.value[:, j, k] - shift[j])
        return out

    def _keys(self, ids):
        return [self.names[int(i)] for i in ids]

    def logpdf_at(self, ids, x):
        return logpdf_point(x, self.desc, self._keys(ids))

    def draws_logpdf(self, ids):
        return logpdf_draws(self.value, self.desc, self._keys(ids))

    def draws_deviance(self, ids, shift):
        D = -2.0 * self.draws_logpdf(ids) - shift
        return np.array([[math.fsum(D[:, k]), math.fsum(D[:, k] ** 2)] for k in range(self.K)])
