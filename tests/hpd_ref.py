"""Restatement of hpd (src/output/stats.jl:54-74) with np.sort, and the inputs of the hpd tests.

hpd(x; alpha): n = length(x); m = max(1, ceil(Int, alpha * n)); y = sort(x); a = y[1:m];
b = y[(n - m + 1):n]; i = the first index of min(b - a); [a[i], b[i]].  hpd(c) applies it to
vec(c.value[:, j, :]) of each monitored param j.

Every input is n x 3 x K (the line model's three monitored values) from a fixed seed.
"""
import math

import numpy as np


def hpd_count(alpha, N):
    return max(1, math.ceil(alpha * float(N)))


def hpd_vec(x, alpha=0.05):
    """([a[i], b[i]], i) with i the 0-based first argmin of b - a."""
    x = np.asarray(x, dtype=np.float64).ravel()
    N = x.size
    m = hpd_count(alpha, N)
    y = np.sort(x)
    a, b = y[:m], y[N - m:]
    i = int(np.argmin(b - a))
    return np.array([a[i], b[i]]), i


def hpd(value, alpha=0.05):
    """(p x 2 intervals, p indices) of an n x p x K draw array."""
    res = [hpd_vec(value[:, j, :], alpha) for j in range(value.shape[1])]
    return np.stack([r[0] for r in res]), np.array([r[1] for r in res], dtype=np.int64)


def input_small(n=41, K=67):
    """N = 2747, m = 138 at alpha 0.05: neither is a multiple of 64 or 256.  Standard normal;
    round(3 normal): massive ties at both thresholds and in the gap minimum; normal times
    2^U{-300..300}: both signs, all 8 key bytes vary."""
    rng = np.random.default_rng(20540)
    v = np.empty((n, 3, K))
    v[:, 0, :] = rng.normal(size=(n, K))
    v[:, 1, :] = np.round(3.0 * rng.normal(size=(n, K)))
    v[:, 2, :] = np.ldexp(rng.normal(size=(n, K)), rng.integers(-300, 301, size=(n, K)))
    return v


def input_flat(n=16, K=130):
    """A constant (interval [c, c], index 0); values in {1, 2}; a series with 0.0 and -0.0."""
    rng = np.random.default_rng(20541)
    v = np.empty((n, 3, K))
    v[:, 0, :] = -2.5
    v[:, 1, :] = rng.integers(1, 3, size=(n, K)).astype(np.float64)
    v[:, 2, :] = rng.choice(np.array([0.0, -0.0, 0.0, -0.0, 1.5, -1.5, 1e-300, -1e-300]), size=(n, K))
    return v


def input_big(n=400, K=257):
    """N = 102800, m = 5140 at alpha 0.05.  A two-component normal mixture (interior argmin);
    gamma(0.7) (argmin at index 0); -gamma(0.7) (argmin at index m - 1)."""
    rng = np.random.default_rng(20542)
    v = np.empty((n, 3, K))
    pick = rng.random(size=(n, K)) < 0.35
    v[:, 0, :] = np.where(pick, rng.normal(-2.0, 0.5, size=(n, K)), rng.normal(1.5, 1.0, size=(n, K)))
    v[:, 1, :] = rng.gamma(0.7, size=(n, K))
    v[:, 2, :] = -rng.gamma(0.7, size=(n, K))
    return v


INPUTS = {"small": input_small, "flat": input_flat, "big": input_big}
