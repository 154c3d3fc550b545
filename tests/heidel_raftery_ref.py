"""heidel_raftery_ref.py — CPU restatement of Mamba's Heidelberger-Welch and Raftery-Lewis
diagnostics and of cor (TEST INFRASTRUCTURE ONLY).

Imported by tests/ as the checker of mamba.jl_amd/diag.py + diag.hip; never by the product.
Restates, on one series or an n x p x m draw array:

  pcramer(q)                         src/utils.jl:73-81
  heideldiag(x; alpha, eps, etype)   src/output/heideldiag.jl:3-27
  rafterydiag(x; q, r, s, eps)       src/output/rafterydiag.jl:3-47
  cor(c)                             src/output/stats.jl:15-17

in the style of diag_ref.py, whose mcse restatement it uses: means and sums of products by
math.fsum (exactly rounded); the running sums B_t of heideldiag.jl:14 are taken on the centred
series in extended precision and their squares summed by fsum.  Divisions follow IEEE (0/0 =
NaN, x/0 = Inf) as Julia's do.

Next to each Heidelberger result come the figures that say how well conditioned a comparison
with another summation order is: the smallest |pvalue - alpha| over the windows tested (inf when
every p-value is NaN), |halfwidth / |mean| - eps| / eps, and the mcse side figures (value_ratio,
margin: see diag_ref) of the second-half and the chosen window.  Next to each Raftery result
comes the smallest |bic| over the thinning steps.

Also here, shared by the CPU and the GPU tests: the AR(1) generator of tests/test_gpu_diag.py
(copied, that file is not edited) and the three inputs A, B, C.
"""
import math

import numpy as np
from scipy import special

import diag_ref

NAN = float("nan")
F64 = np.float64


# ---------------------------------------------------------------- inputs
def ar1(n, K, seed=1, phis=(0.3, 0.6, 0.9), shift=(0.0, 25.0, -1000.0)):
    """n x 3 x K AR(1) series x_t = phi x_{t-1} + e_t, one phi per param, on distinct levels."""
    e = np.random.default_rng(seed).normal(size=(n, 3, K))
    x = np.empty_like(e)
    ph = np.asarray(phis)[:, None]
    x[0] = e[0]
    for t in range(1, n):
        x[t] = ph * x[t - 1] + e[t]
    return x + np.asarray(shift)[None, :, None]


def with_transient(x):
    """Chains 0-7 start 6 above their level and decay over 0.08 n iterations: later starts and
    non-convergence occur."""
    n = x.shape[0]
    x = x.copy()
    x[:, :, :8] += (6.0 * np.exp(-np.arange(n) / (0.08 * n)))[:, None, None]
    return x


def input_a():
    """400 x 3 x 96: one full and one partial wavefront."""
    return with_transient(ar1(400, 96, seed=1))


def input_b():
    """57 x 3 x 70: an odd length that is no multiple of any unroll."""
    return with_transient(ar1(57, 70, seed=5))


def input_c():
    """400 x 3 x 70 AR(1) rounded to integers (ties at the threshold), chain 0 constant 1.5."""
    x = np.round(ar1(400, 70, seed=8, shift=(0.0, 3.0, -7.0)))
    x[:, :, 0] = 1.5
    return x


def input_n19():
    """19 x 3 x 66: the length with the most candidate windows (9)."""
    return ar1(19, 66, seed=6)


# ---------------------------------------------------------------- Heidelberger and Welch
def pcramer(q):
    """utils.jl:73-81."""
    with np.errstate(all="ignore"):
        q = F64(q)
        p = F64(0.0)
        for k in range(4):
            c1 = 4.0 * k + 1.0
            c2 = F64(c1 ** 2) / (16.0 * q)
            p = p + special.gamma(k + 0.5) / math.factorial(k) * math.sqrt(c1) * np.exp(-c2) * special.kv(0.25, c2)
        return float(p / (math.pi ** 1.5 * np.sqrt(q)))


def cvm(y):
    """(mean, W) of one window: W = sum_t B_t^2 / m^2, B_t = sum_{u<=t} (y_u - mean): sum(Bsq) / m of
    heideldiag.jl:13-16 without the 1 / S0."""
    mu, z = diag_ref.centred(y)
    m = z.size
    B = np.cumsum(z.astype(np.longdouble))
    return mu, math.fsum((B * B).astype(np.float64)) / (float(m) * float(m))


def heidel_starts(n):
    """heideldiag.jl:6-10, 22: the 0-based candidate starts and the first 1-based i >= n / 2."""
    delta = int(0.10 * n)
    starts, i = [], 1
    while i < n / 2:
        starts.append(i - 1)
        i += delta
    return starts, i


def heideldiag(x, alpha=0.05, eps=0.1, etype="imse", size=100, start=1):
    """heideldiag.jl:3-27 -> (the six figures, side figures dict)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    if n < 10:
        raise ValueError("heideldiag needs at least 10 iterations")
    delta = int(0.10 * n)
    h0 = int(n / 2) - 1
    r0 = diag_ref.mcse(x[h0:], etype, size)
    with np.errstate(all="ignore"):
        S0 = F64(n - h0) * F64(r0["mcse"]) ** 2
        i, pvalue, converged, ybar, s = 1, 1.0, False, NAN, 0
        gap = math.inf
        while i < n / 2:
            s = i - 1
            ybar, W = cvm(x[s:])
            pvalue = 1.0 - pcramer(F64(W) / S0)
            if not math.isnan(pvalue):
                gap = min(gap, abs(pvalue - alpha))
            converged = pvalue > alpha
            if converged:
                break
            i += delta
        rc = diag_ref.mcse(x[s:], etype, size)
        halfwidth = math.sqrt(2.0) * float(special.erfinv(1.0 - alpha)) * rc["mcse"]
        ratio = F64(halfwidth) / F64(abs(ybar))
        passed = bool(ratio <= eps)
    side = dict(pgap=gap, hwgap=abs(float(ratio) - eps) / eps if not math.isnan(ratio) else math.inf,
                value_ratio=np.min([r0["value_ratio"], rc["value_ratio"]]),   # NaN (constant) propagates
                margin=min(r0["margin"], rc["margin"]), start=s)
    return [float(i + start - 2), float(converged), float(np.round(pvalue, 4)), ybar, halfwidth, float(passed)], side


def heideldiag_chains(value, alpha=0.05, eps=0.1, etype="imse", size=100, start=1):
    """heideldiag.jl:29-41: (p x 6 x m, dict of p x m side figures)."""
    value = np.asarray(value, dtype=np.float64)
    _, p, m = value.shape
    vals = np.empty((p, 6, m))
    side = {k: np.empty((p, m)) for k in ("pgap", "hwgap", "value_ratio", "margin", "start")}
    for j in range(p):
        for k in range(m):
            vals[j, :, k], sd = heideldiag(value[:, j, k], alpha, eps, etype, size, start)
            for key in side:
                side[key][j, k] = sd[key]
    return vals, side


def window_cvm(value, starts):
    """m x p x nstarts x [mean, W] of the suffix windows (mmb_chain_cvm's layout)."""
    value = np.asarray(value, dtype=np.float64)
    _, p, m = value.shape
    out = np.empty((m, p, len(starts), 2))
    for k in range(m):
        for j in range(p):
            for q, s in enumerate(starts):
                out[k, j, q] = cvm(value[s:, j, k])
    return out


def window_mcse_from(value, i0, i1, etype="imse", size=100):
    """diag_ref.window_mcse with a start per (chain, param), i0 m x p (mmb_chain_mcse_from's
    layout): fields m x p x 4 and the side figures value_ratio, margin."""
    value = np.asarray(value, dtype=np.float64)
    _, p, m = value.shape
    out = np.empty((m, p, 4))
    ratio = np.empty((m, p))
    margin = np.empty((m, p))
    for k in range(m):
        for j in range(p):
            r = diag_ref.mcse(value[int(i0[k][j]):i1, j, k], etype, size)
            out[k, j] = [r["mean"], r["gamma0"], r["mcse"], r["terms"]]
            ratio[k, j], margin[k, j] = r["value_ratio"], r["margin"]
    return out, ratio, margin


# ---------------------------------------------------------------- Raftery and Lewis
def quantile(x, q):
    """Julia 0.5 quantile(x, q) (mamba.jl_amd/summary.py quantile_sharded restates the same)."""
    s = np.sort(np.asarray(x, dtype=np.float64))
    index = 1.0 + (s.size - 1) * q
    lo, hi = math.floor(index), math.ceil(index)
    h = index - lo
    a, b = s[lo - 1], s[hi - 1]
    return float(a if index == lo else (1.0 - h) * a + h * b)


def raftery_counts(x, q):
    """rafterydiag.jl:13-34 -> ([threshold, kthin, ntest, n00, n10, n01, n11, bic], smallest |bic|).
    A series whose thinned sequence runs out (ntest < 3: the reference's log(-1)) gets kthin and
    bic NaN and zero counts."""
    x = np.asarray(x, dtype=np.float64)
    thr = quantile(x, q)
    dichot = (x <= thr).astype(np.int64)
    kthin, least = 0, math.inf
    while True:
        kthin += 1
        test = dichot[::kthin]
        ntest = test.size
        if ntest < 3:
            return [thr, NAN, float(ntest), 0.0, 0.0, 0.0, 0.0, NAN], least
        T = np.bincount(test[:-2] + 2 * test[1:-1] + 4 * test[2:], minlength=8).reshape(2, 2, 2).T  # T[i1, i2, i3]
        g2 = 0.0
        for i1 in range(2):
            for i2 in range(2):
                for i3 in range(2):
                    tt = int(T[i1, i2, i3])
                    if tt > 0:
                        fitted = float(int(T[:, i2, i3].sum()) * int(T[i1, i2, :].sum())) / float(int(T[:, i2, :].sum()))
                        g2 += 2.0 * tt * math.log(tt / fitted)
        bic = g2 - 2.0 * math.log(ntest - 2.0)
        least = min(least, abs(bic))
        if not bic >= 0.0:
            break
    tf = np.bincount(test[:-1] + 2 * test[1:], minlength=4)
    return [thr, float(kthin), float(ntest), float(tf[0]), float(tf[1]), float(tf[2]), float(tf[3]), bic], least


def raftery_nmin(q, r, s):
    phi = math.sqrt(2.0) * float(special.erfinv(s))
    return phi, int(math.ceil(q * (1.0 - q) * ((phi / r) * (phi / r))))


def rafterydiag(x, q=0.025, r=0.005, s=0.95, eps=0.001, start=1, thin=1):
    """rafterydiag.jl:3-47 -> ([kthin, burnin, total, nmin, total / nmin], smallest |bic|); the
    caller issues the warning of line 10."""
    phi, nmin = raftery_nmin(q, r, s)
    if nmin > len(x):
        return [NAN, NAN, NAN, float(nmin), NAN], math.inf
    f, least = raftery_counts(x, q)
    with np.errstate(all="ignore"):
        n00, n10, n01, n11 = (F64(v) for v in f[3:7])
        alpha = n01 / (n00 + n01)
        beta = n10 / (n10 + n11)
        kthin = F64(f[1]) * thin
        ab = alpha + beta
        m = np.log(eps * ab / np.maximum(alpha, beta)) / np.log(np.abs(1.0 - alpha - beta))
        burnin = kthin * np.ceil(m) + start - 1
        nn = ((2.0 - alpha - beta) * alpha * beta * (phi * phi)) / ((r * r) * (ab * ab * ab))
        total = burnin + kthin * np.ceil(nn)
        return [float(kthin), float(burnin), float(total), float(nmin), float(total / nmin)], least


def rafterydiag_chains(value, q=0.025, r=0.005, s=0.95, eps=0.001, start=1, thin=1):
    """rafterydiag.jl:49-61: (p x 5 x m, smallest |bic| p x m)."""
    value = np.asarray(value, dtype=np.float64)
    _, p, m = value.shape
    vals = np.empty((p, 5, m))
    least = np.empty((p, m))
    for j in range(p):
        for k in range(m):
            vals[j, :, k], least[j, k] = rafterydiag(value[:, j, k], q, r, s, eps, start, thin)
    return vals, least


def window_raftery(value, q):
    """m x p x 8 (mmb_chain_raftery's layout) and the smallest |bic| m x p."""
    value = np.asarray(value, dtype=np.float64)
    _, p, m = value.shape
    out = np.empty((m, p, 8))
    least = np.empty((m, p))
    for k in range(m):
        for j in range(p):
            out[k, j], least[k, j] = raftery_counts(value[:, j, k], q)
    return out, least


# ---------------------------------------------------------------- cor
def cor(value):
    """cor(combine(c)) (stats.jl:15-17): the chains stacked into (n m) x p, Pearson correlation."""
    value = np.asarray(value, dtype=np.float64)
    n, p, m = value.shape
    pooled = value.transpose(0, 2, 1).reshape(n * m, p)
    z = np.stack([pooled[:, j] - math.fsum(pooled[:, j]) / (n * m) for j in range(p)], axis=1)
    ss = np.array([[math.fsum(z[:, i] * z[:, j]) for j in range(p)] for i in range(p)])
    out = ss / np.sqrt(np.outer(np.diag(ss), np.diag(ss)))
    out[np.diag_indices(p)] = 1.0
    return out


# ---------------------------------------------------------------- engine-shaped host shard
class HostShard(diag_ref.HostDiagShard):
    """diag_ref.HostDiagShard with the partials of mmb_chain_cvm / mmb_chain_mcse_from /
    mmb_chain_raftery (include/mamba_hip.h)."""

    def chain_cvm(self, starts):
        return window_cvm(self.d, [int(s) for s in starts])

    def chain_mcse_from(self, i0, i1, etype, batch_size=100):
        name = {0: "bm", 1: "imse", 2: "ipse"}.get(etype, etype)
        return window_mcse_from(self.d, np.asarray(i0), i1, name, batch_size)[0]

    def chain_raftery(self, q):
        return window_raftery(self.d, q)[0]
