"""diag_ref.py — CPU restatement of Mamba's per-chain diagnostics (TEST INFRASTRUCTURE ONLY).

Imported by tests/ as the checker of mamba.jl_amd/diag.py + diag.hip; never by the product.
Restates, on an n x p x m draw array (or one series):

  autocor(c; lags, relative)     src/output/stats.jl:3-13   -> StatsBase autocor(x, lags)
  changerate(c)                  src/output/stats.jl:19-39
  mcse(x, method)                src/output/mcse.jl:3-8
  mcse_bm(x; size)               src/output/mcse.jl:10-19
  mcse_imse(x)                   src/output/mcse.jl:21-33
  mcse_ipse(x)                   src/output/mcse.jl:35-46
  gewekediag(x; first, last)     src/output/gewekediag.jl:3-18

StatsBase 0.7 (not vendored; recalled): autocov(x, lags; demean=true)[l] =
sum_{t} z_t z_{t+l} / length(x) with z = x - mean(x); autocor = autocov / autocov at lag 0; a lag
>= length(x) is an error ("lags must be less than the sample length").

Sums use math.fsum (exactly rounded).  A series whose elements are all equal is centred to
z = 0 exactly, so every gamma(l) is 0: mcse 0, autocor and Geweke z 0/0 = NaN.  Where the
reference's sqrt would throw a DomainError (negative `value`) the result is NaN.

Next to each IMSE / IPSE result two side figures say how well conditioned the comparison with
another summation order is: value / gamma(0), and the smallest |Ghat| / gamma(0) over the
`Ghat > 0 || break` decisions (inf when the loop made none).
"""
import math

import numpy as np

NAN = float("nan")


def centred(x):
    """(mean, z) with z = x - mean(x); exactly zero for a series of equal elements."""
    x = np.asarray(x, dtype=np.float64)
    if np.all(x == x[0]):
        return float(x[0]), np.zeros_like(x)
    mu = math.fsum(x) / x.size
    return mu, x - mu


def autocov(x, lags):
    """StatsBase autocov(x, lags; demean=true)."""
    mu, z = centred(x)
    n = z.size
    out = []
    for l in lags:
        if not 0 <= l < n:
            raise ValueError("lags must be less than the sample length")
        out.append(math.fsum(z[:n - l] * z[l:]) / n)
    return out


def _sqrt(v):
    return math.sqrt(v) if v >= 0.0 else NAN   # Julia: DomainError for v < 0; sqrt(-0.0) = -0.0


def _ratio(a, g0):
    return a / g0 if g0 != 0.0 else NAN


def mcse_imse(x):
    """mcse.jl:21-33 -> dict(mcse, mean, gamma0, terms, value_ratio, margin)."""
    n = len(x)
    m = (n - 2) // 2 if n >= 2 else 0          # div(n - 2, 2)
    ghat = autocov(x, [0, 1])
    Ghat = ghat[0] + ghat[1]
    value = -ghat[0] + 2 * Ghat
    terms, margin = 0, math.inf
    for i in range(1, m + 1):
        Ghat = min(Ghat, sum(autocov(x, [2 * i, 2 * i + 1])))
        if ghat[0] != 0.0:
            margin = min(margin, abs(Ghat) / ghat[0])
        if not Ghat > 0:
            break
        value += 2 * Ghat
        terms += 1
    return dict(mcse=_sqrt(value / n), mean=centred(x)[0], gamma0=ghat[0], terms=terms,
                value_ratio=_ratio(value, ghat[0]), margin=margin)


def mcse_ipse(x):
    """mcse.jl:35-46."""
    n = len(x)
    m = (n - 2) // 2 if n >= 2 else 0
    ghat = autocov(x, [0, 1])
    value = ghat[0] + 2 * ghat[1]
    terms, margin = 0, math.inf
    for i in range(1, m + 1):
        Ghat = sum(autocov(x, [2 * i, 2 * i + 1]))
        if ghat[0] != 0.0:
            margin = min(margin, abs(Ghat) / ghat[0])
        if not Ghat > 0:
            break
        value += 2 * Ghat
        terms += 1
    return dict(mcse=_sqrt(value / n), mean=centred(x)[0], gamma0=ghat[0], terms=terms,
                value_ratio=_ratio(value, ghat[0]), margin=margin)


def mcse_bm(x, size=100):
    """mcse.jl:10-19 on the centred series (sem is shift-invariant)."""
    n = len(x)
    m = n // size
    if m < 2:
        raise ValueError(f"iterations are < {2 * size} and batch size is > {n // 2}")
    mu, z = centred(x)
    mbar = [math.fsum(z[i * size:(i + 1) * size]) / size for i in range(m)]
    mb = math.fsum(mbar) / m
    sd = math.sqrt(math.fsum((b - mb) ** 2 for b in mbar) / (m - 1))
    g0 = math.fsum(z * z) / n
    return dict(mcse=sd / math.sqrt(m), mean=mu, gamma0=g0, terms=m, value_ratio=math.inf, margin=math.inf)


def mcse(x, etype="imse", size=100):
    """mcse.jl:3-8."""
    if etype == "bm":
        return mcse_bm(x, size)
    if etype == "imse":
        return mcse_imse(x)
    if etype == "ipse":
        return mcse_ipse(x)
    raise ValueError(f"unsupported mcse method {etype}")


def window_mcse(value, i0, i1, etype="imse", size=100):
    """Every (chain, param) series of value[i0:i1]: fields m x p x [mean, gamma0, mcse, terms]
    (the layout of mmb_chain_mcse) and the side figures value_ratio, margin (m x p)."""
    value = np.asarray(value, dtype=np.float64)
    _, p, m = value.shape
    out = np.empty((m, p, 4))
    ratio = np.empty((m, p))
    margin = np.empty((m, p))
    for k in range(m):
        for j in range(p):
            r = mcse(value[i0:i1, j, k], etype, size)
            out[k, j] = [r["mean"], r["gamma0"], r["mcse"], r["terms"]]
            ratio[k, j], margin[k, j] = r["value_ratio"], r["margin"]
    return out, ratio, margin


def window_autocov(value, i0, i1, lags):
    """m x p x (2 + nlags): [mean, gamma(0), gamma(lags[0]), ...] (mmb_chain_autocov's layout)."""
    value = np.asarray(value, dtype=np.float64)
    _, p, m = value.shape
    out = np.empty((m, p, 2 + len(lags)))
    for k in range(m):
        for j in range(p):
            x = value[i0:i1, j, k]
            out[k, j] = [centred(x)[0]] + autocov(x, [0] + list(lags))
    return out


def autocor(value, lags=(1, 5, 10, 50), thin=1, relative=True):
    """stats.jl:3-13: (p x nlags x m, labels)."""
    lags = [int(l) for l in lags]
    if relative:
        lags = [l * thin for l in lags]
    elif any(l % thin != 0 for l in lags):
        raise ValueError("lags do not correspond to thinning interval")
    value = np.asarray(value, dtype=np.float64)
    n, p, m = value.shape
    out = np.empty((p, len(lags), m))
    for k in range(m):
        for j in range(p):
            g = autocov(value[:, j, k], [0] + lags)
            out[j, :, k] = [gl / g[0] if g[0] != 0.0 else NAN for gl in g[1:]]
    return out, [f"Lag {l}" for l in lags]


def change_counts(value):
    """The counts of stats.jl:19-36 before the division: p per-param counts, then r_mv."""
    value = np.asarray(value, dtype=np.float64)
    n, p, m = value.shape
    r = np.zeros(p + 1, dtype=np.int64)
    for k in range(m):
        prev = value[0, :, k].copy()
        for i in range(1, n):
            anyd = False
            for j in range(p):
                x = value[i, j, k]
                dx = bool(x != prev[j])
                r[j] += dx
                anyd |= dx
                prev[j] = x
            r[p] += anyd
    return r


def changerate(value):
    """stats.jl:19-39: round([r; r_mv] / (m * (n - 1)), 3)."""
    n, _, m = np.shape(value)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.round(change_counts(value) / float(m * (n - 1)), 3)


def geweke_windows(n, first=0.1, last=0.5):
    """gewekediag.jl:13-14 as 0-based half-open ranges (round: ties to even, Julia's round)."""
    return (0, int(round(first * n))), (int(round(n - last * n + 1)) - 1, n)


def geweke_z(x, first=0.1, last=0.5, etype="imse", size=100):
    """gewekediag.jl:5-16 -> (z, [mcse dicts of the two windows])."""
    if not 0.0 < first < 1.0:
        raise ValueError("first is not in (0, 1)")
    if not 0.0 < last < 1.0:
        raise ValueError("last is not in (0, 1)")
    if first + last > 1.0:
        raise ValueError("first and last proportions overlap")
    (a0, a1), (b0, b1) = geweke_windows(len(x), first, last)
    r1, r2 = mcse(x[a0:a1], etype, size), mcse(x[b0:b1], etype, size)
    with np.errstate(invalid="ignore", divide="ignore"):   # 0/0 = NaN, x/0 = Inf as in Julia
        z = float((np.float64(r1["mean"]) - r2["mean"]) / np.sqrt(np.float64(r1["mcse"]) ** 2 + r2["mcse"] ** 2))
    return z, [r1, r2]


def gewekediag(value, first=0.1, last=0.5, etype="imse", size=100):
    """gewekediag.jl:17-31: (p x 2 x m [round(z, 3), round(1 - erf(|z|/sqrt(2)), 4)], unrounded z
    p x m, the smaller value_ratio and margin of the two windows p x m)."""
    value = np.asarray(value, dtype=np.float64)
    _, p, m = value.shape
    vals = np.empty((p, 2, m))
    zs = np.empty((p, m))
    ratio = np.empty((p, m))
    margin = np.empty((p, m))
    for j in range(p):
        for k in range(m):
            z, rs = geweke_z(value[:, j, k], first, last, etype, size)
            zs[j, k] = z
            pv = 1.0 - math.erf(abs(z) / math.sqrt(2.0)) if not math.isnan(z) else NAN
            vals[j, :, k] = [np.round(z, 3), np.round(pv, 4)]
            ratio[j, k] = np.min([r["value_ratio"] for r in rs])   # NaN (constant window) propagates
            margin[j, k] = np.min([r["margin"] for r in rs])
    return vals, zs, ratio, margin


class HostDiagShard:
    """Engine-shaped view of n x p x k draws whose partials restate the contracts of
    mmb_chain_autocov / mmb_chain_mcse / mmb_change_counts (include/mamba_hip.h)."""

    def __init__(self, draws):
        self.d = np.asarray(draws, dtype=np.float64)
        self.pmon, self.K = self.d.shape[1], self.d.shape[2]

    def num_kept(self):
        return self.d.shape[0]

    def chain_autocov(self, i0, i1, lags):
        return window_autocov(self.d, i0, i1, lags)

    def chain_mcse(self, i0, i1, etype, batch_size=100):
        name = {0: "bm", 1: "imse", 2: "ipse"}.get(etype, etype)
        return window_mcse(self.d, i0, i1, name, batch_size)[0]

    def change_counts(self):
        return change_counts(self.d)
