"""Per-chain convergence diagnostics of the device-kept draws.

autocor and changerate (src/output/stats.jl:3-39), gewekediag (src/output/gewekediag.jl) and
mcse (src/output/mcse.jl:3-46) look at one chain at a time: its mixing (autocorrelation, how
often it moved) and its within-chain drift (Geweke).  The per-element work runs on the GPU
(diag.hip through mmb_chain_autocov / mmb_chain_mcse / mmb_change_counts); this module checks
the arguments as the reference does, picks the windows and applies the closing formulas to the
K x p partials.

`engine` is anything engine-shaped: num_kept(), K, pmon, chain_autocov(i0, i1, lags),
chain_mcse(i0, i1, etype, batch_size) and change_counts().

Rounding: Julia's round (round(Int, x) for the Geweke windows, round(x, digits) for the
reported figures) rounds to nearest with ties to even, as Python's round and numpy's do.
"""
import math

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
