"""Per-chain convergence diagnostics of the device-kept draws.

autocor and changerate (src/output/stats.jl:3-39), gewekediag (src/output/gewekediag.jl) and
mcse (src/output/mcse.jl:3-46) look at one chain at a time: its mixing (autocorrelation, how
often it moved) and its within-chain drift (Geweke).  The per-element work runs on the GPU
(diag.hip through mmb_chain_autocov / mmb_chain_mcse / mmb_change_counts); this module checks
the arguments as the reference does, picks the windows and applies the closing formulas to the
K x p partials.

heideldiag (src/output/heideldiag.jl:3-27) and rafterydiag (src/output/rafterydiag.jl:3-47)
are per-chain too.  Their per-element work is mmb_chain_cvm / mmb_chain_mcse_from /
mmb_chain_raftery; what stays here is the Cramer-von Mises distribution function (pcramer,
src/utils.jl:73-81, with scipy.special), the choice of each series' window, and the closing
formulas, all vectorised over K x p with IEEE semantics (0/0 = NaN, x/0 = Inf, as Julia's float
division gives them).

`engine` is anything engine-shaped: num_kept(), K, pmon, chain_autocov(i0, i1, lags),
chain_mcse(i0, i1, etype, batch_size) and change_counts(); for the last two diagnostics also
chain_cvm(starts), chain_mcse_from(i0, i1, etype, batch_size) and chain_raftery(q).

Rounding: Julia's round (round(Int, x) for the Geweke windows, round(x, digits) for the
reported figures) rounds to nearest with ties to even, as Python's round and numpy's do.
Julia 0.5's round(x, digits) is round(x * 10^digits) / 10^digits; np.round computes the same
three operations (scale, rint, unscale), so the rounded p-values are the reference's for the
same unrounded value.

Departures from the reference, beyond NaN for a DomainError: heideldiag refuses fewer than 10
draws (delta = trunc(0.10 n) is then 0 and the reference's loop never ends for a series that
does not converge at its first window); rafterydiag reports NaN for a series whose thinned
test sequence drops below 3 elements before bic turns negative (the reference: DomainError
from log(-1)).
"""
import math
import warnings

import numpy as np

from . import abi
from .samplers import ArgumentError

ETYPES = {"bm": abi.MMB_MCSE_BM, "imse": abi.MMB_MCSE_IMSE, "ipse": abi.MMB_MCSE_IPSE}
F_MEAN, F_GAMMA0, F_MCSE, F_TERMS = range(4)


def etype_code(etype):
    """:bm / :imse / :ipse (mcse.jl:3-8) -> MMB_MCSE_*."""
    key = str(etype).lstrip(":")
    if key not in ETYPES:
        raise ArgumentError(f"unsupported mcse method {etype}")
    return ETYPES[key]


def _check_mcse_window(nw, code, batch_size):
    if code == abi.MMB_MCSE_BM:
        if batch_size < 1:
            raise ArgumentError("batch size must be positive")
        if nw // batch_size < 2:  # mcse.jl:13-16
            raise ArgumentError(f"iterations are < {2 * batch_size} and batch size is > {nw // 2}")
    elif nw < 2:                  # autocov(x, [0, 1]) of a single element (StatsBase)
        raise ArgumentError("lags must be less than the sample length")


def index_lags(lags, thin=1, relative=True):
    """The lags autocor hands to StatsBase (stats.jl:5-9): `relative` multiplies them by the
    thinning interval, otherwise each must be a multiple of it."""
    lags = [int(x) for x in lags]
    thin = int(thin)
    if relative:
        lags = [x * thin for x in lags]
    elif any(x % thin != 0 for x in lags):
        raise ArgumentError("lags do not correspond to thinning interval")
    return lags


def autocor(engine, lags=(1, 5, 10, 50), thin=1, relative=True):
    """autocor(c; lags, relative) (stats.jl:3-13) per chain: (p x nlags x K values, labels).
    The lags of `index_lags` are used as index lags of the kept series, as the reference does."""
    lags = index_lags(lags, thin, relative)
    n = engine.num_kept()
    if any(x < 1 or x >= n for x in lags):
        raise ArgumentError("lags must be less than the sample length")
    out = np.empty((engine.pmon, len(lags), engine.K))
    for c0 in range(0, len(lags), abi.MMB_DIAG_MAX_LAGS):
        chunk = lags[c0:c0 + abi.MMB_DIAG_MAX_LAGS]
        ac = engine.chain_autocov(0, n, chunk)                 # K x p x (2 + len(chunk))
        with np.errstate(invalid="ignore", divide="ignore"):
            r = ac[:, :, 2:] / ac[:, :, 1:2]                   # gamma(l) / gamma(0); constant chain: 0/0
        out[:, c0:c0 + len(chunk), :] = r.transpose(1, 2, 0)
    return out, [f"Lag {x}" for x in lags]


def changerate_sharded(engine, allreduce_sum=None):
    """changerate(c) (stats.jl:19-39) over every chain of every rank: the p + 1 rates
    [params..., Multivariate] = counts / (m (n - 1)), rounded to 3 decimals.  The counts and
    the chain count are additive: one sum all-reduce."""
    v = np.concatenate([np.asarray(engine.change_counts(), dtype=np.float64), [float(engine.K)]])
    if allreduce_sum is not None:
        v = np.asarray(allreduce_sum(v), dtype=np.float64)
    counts, m, n = np.rint(v[:-1]), int(round(v[-1])), engine.num_kept()
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.round(counts / float(m * (n - 1)), 3)


def geweke_windows(n, first=0.1, last=0.5):
    """The two windows of gewekediag.jl:13-14 as 0-based half-open ranges:
    x[1:round(Int, first*n)] and x[round(Int, n - last*n + 1):n]."""
    if not 0.0 < first < 1.0:
        raise ArgumentError("first is not in (0, 1)")
    if not 0.0 < last < 1.0:
        raise ArgumentError("last is not in (0, 1)")
    if first + last > 1.0:
        raise ArgumentError("first and last proportions overlap")
    # round: ties to even, Julia's round(Int, x)
    return (0, int(round(first * n))), (int(round(n - last * n + 1)) - 1, n)


def geweke_z(engine, first=0.1, last=0.5, etype="imse", batch_size=100):
    """The unrounded Geweke z (gewekediag.jl:15-16) per param and chain, p x K:
    (mean(x1) - mean(x2)) / sqrt(mcse(x1)^2 + mcse(x2)^2)."""
    code = etype_code(etype)
    n = engine.num_kept()
    w1, w2 = geweke_windows(n, first, last)
    for a, b in (w1, w2):
        if b <= a:
            raise ArgumentError(f"empty window: {n} iterations with first = {first}, last = {last}")
        _check_mcse_window(b - a, code, batch_size)
    a = engine.chain_mcse(w1[0], w1[1], code, batch_size)
    b = engine.chain_mcse(w2[0], w2[1], code, batch_size)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = (a[:, :, F_MEAN] - b[:, :, F_MEAN]) / np.sqrt(a[:, :, F_MCSE] ** 2 + b[:, :, F_MCSE] ** 2)
    return z.T


def gewekediag(engine, first=0.1, last=0.5, etype="imse", batch_size=100):
    """gewekediag(c) (gewekediag.jl:20-31): p x 2 x K, [round(z, 3), round(1 - erf(|z|/sqrt(2)), 4)]."""
    z = geweke_z(engine, first, last, etype, batch_size)
    pv = 1.0 - np.vectorize(math.erf, otypes=[float])(np.abs(z) / math.sqrt(2.0))
    return np.stack([np.round(z, 3), np.round(pv, 4)], axis=1)


def mcse(engine, etype="imse", batch_size=100):
    """mcse(x, etype) (mcse.jl:3-8) of every chain's whole kept series: p x K."""
    code = etype_code(etype)
    n = engine.num_kept()
    _check_mcse_window(n, code, batch_size)
    return engine.chain_mcse(0, n, code, batch_size)[:, :, F_MCSE].T


def pcramer(q):
    """pcramer(q) (utils.jl:73-81): the distribution function of the Cramer-von Mises statistic,
    the first four terms of its series; elementwise over an array."""
    from scipy import special
    q = np.asarray(q, dtype=np.float64)
    p = np.zeros_like(q)
    with np.errstate(all="ignore"):
        for k in range(4):
            c1 = 4.0 * k + 1.0
            c2 = c1 * c1 / (16.0 * q)
            p = p + special.gamma(k + 0.5) / math.factorial(k) * math.sqrt(c1) * np.exp(-c2) * special.kv(0.25, c2)
        return p / (math.pi ** 1.5 * np.sqrt(q))


def heidel_starts(n):
    """The candidate windows of heideldiag.jl:6-10, 22: (0-based starts s_j = j delta of the
    1-based i = 1, 1 + delta, ... < n / 2, and the first i >= n / 2)."""
    delta = int(0.10 * n)                       # trunc(Int, 0.10 * n)
    starts, i = [], 1
    while i < n / 2:
        starts.append(i - 1)
        i += delta
    return starts, i


def heideldiag(engine, alpha=0.05, eps=0.1, etype="imse", batch_size=100, start=1):
    """heideldiag(c; alpha, eps, etype, start) (heideldiag.jl:3-27): p x 6 x K, [Burn-in,
    Stationarity, p-value, Mean, Halfwidth, Test].  A series that never converges keeps the
    p-value, mean and halfwidth of the last window tested and reports the first i >= n / 2."""
    from scipy import special
    code = etype_code(etype)
    n = engine.num_kept()
    if n < 10:
        raise ArgumentError(f"heideldiag needs at least 10 iterations, got {n}")
    h0 = int(n / 2) - 1                         # x[trunc(Int, n / 2):end], 0-based
    _check_mcse_window(n - h0, code, batch_size)  # the shortest window any series gets
    starts, i_final = heidel_starts(n)
    half = engine.chain_mcse(h0, n, code, batch_size)
    cv = engine.chain_cvm(starts)               # K x p x candidates x [mean, W]
    with np.errstate(all="ignore"):
        S0 = (n - h0) * half[:, :, F_MCSE] ** 2
        pv = 1.0 - pcramer(cv[:, :, :, 1] / S0[:, :, None])
        conv = pv > alpha                       # NaN: not converged
        ok = conv.any(axis=2)
        sel = np.where(ok, conv.argmax(axis=2), len(starts) - 1)
        s_sel = np.asarray(starts, dtype=np.int64)[sel]
        pvalue = np.take_along_axis(pv, sel[:, :, None], axis=2)[:, :, 0]
        ybar = np.take_along_axis(cv[:, :, :, 0], sel[:, :, None], axis=2)[:, :, 0]
        m = engine.chain_mcse_from(s_sel, n, code, batch_size)
        halfwidth = math.sqrt(2.0) * float(special.erfinv(1.0 - alpha)) * m[:, :, F_MCSE]
        passed = halfwidth / np.abs(ybar) <= eps
        burnin = np.where(ok, s_sel + 1, i_final) + start - 2
        out = np.stack([burnin.astype(np.float64), ok.astype(np.float64), np.round(pvalue, 4), ybar, halfwidth,
                        passed.astype(np.float64)], axis=2)
    return out.transpose(1, 2, 0)


def raftery_nmin(q, r, s):
    """(phi, nmin) of rafterydiag.jl:7-8."""
    from scipy import special
    phi = math.sqrt(2.0) * float(special.erfinv(s))
    return phi, int(math.ceil(q * (1.0 - q) * ((phi / r) * (phi / r))))


def raftery_from_counts(kthin, n00, n10, n01, n11, phi, nmin, r, eps, start=1, thin=1):
    """rafterydiag.jl:35-46 on the final transition counts: [kthin, burnin, total, nmin,
    total / nmin] along a new last axis."""
    with np.errstate(all="ignore"):
        alpha = n01 / (n00 + n01)
        beta = n10 / (n10 + n11)
        kthin = kthin * thin
        ab = alpha + beta
        m = np.log(eps * ab / np.maximum(alpha, beta)) / np.log(np.abs(1.0 - alpha - beta))
        burnin = kthin * np.ceil(m) + start - 1
        nn = ((2.0 - alpha - beta) * alpha * beta * (phi * phi)) / ((r * r) * (ab * ab * ab))
        total = burnin + kthin * np.ceil(nn)
        return np.stack([kthin, burnin, total, np.full_like(total, float(nmin)), total / nmin], axis=-1)


def rafterydiag(engine, q=0.025, r=0.005, s=0.95, eps=0.001, start=1, thin=1):
    """rafterydiag(c; q, r, s, eps) (rafterydiag.jl:3-47): p x 5 x K, [Thinning, Burn-in, Total,
    Nmin, Dependence Factor]."""
    if not 0.0 < q < 1.0:
        raise ArgumentError("q is not in (0, 1)")
    if not 0.0 < s < 1.0:
        raise ArgumentError("s is not in (0, 1)")
    if not r > 0.0:
        raise ArgumentError("r must be positive")
    if not eps > 0.0:
        raise ArgumentError("eps must be positive")
    n = engine.num_kept()
    phi, nmin = raftery_nmin(q, r, s)
    if nmin > n:
        warnings.warn(f"At least {nmin} samples are needed for specified q, r, and s")
        out = np.full((engine.pmon, 5, engine.K), np.nan)
        out[:, 3, :] = nmin
        return out
    rf = engine.chain_raftery(q)                # K x p x [threshold, kthin, ntest, n00, n10, n01, n11, bic]
    out = raftery_from_counts(rf[:, :, 1], rf[:, :, 3], rf[:, :, 4], rf[:, :, 5], rf[:, :, 6], phi, nmin, r, eps,
                              start, thin)
    return out.transpose(1, 2, 0)
