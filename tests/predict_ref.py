"""Restatement of the posterior predictive draws (include/mamba_hip.h, "Posterior predictive draws";
predict(mc, nodekeys), src/output/modelstats.jl:71-102) in Python.

Built only on the primitives tests/oracle_lib.py loads -- L.orc_uniform, L.orc_normal, L.orc_log,
L.orc_exp, L.orc_log1p: Philox uniforms and Box-Muller normals of a substream and the exact
elementary functions -- plus IEEE + - * / sqrt on Python floats.  The samplers themselves
(sequential-search inversion for Binomial and Poisson, Marsaglia-Tsang with running indices for
the gamma-based families) are written out here, not called.

A predicted value is a pure function of (seed, global chain id, iteration, node id n, element e):
    node block PB(n) = 256 + n;  element block GB(n, e) = (n + 1) * 65536 + e
`sample` returns (value, edge): edge is True when a discrete draw's uniform lies within EDGE_RTOL
relative of a step of the cdf it was compared with -- there a one-ulp difference in the parameter
could change the count.  Fixtures with no edge draw can be compared exactly.

A model description is a dict
    "cols":  node name -> monitored column indices of the n x p x K value array
    "nodes": observed node name -> {"id": engine node id, "fam": family name, "len": elements,
             "params": f(vals) -> (a, b), arrays of `len` (or scalars), Distributions order}
Parameters are evaluated as modelstats_ref.py evaluates them (numpy on the draw's values).
"""
import math

import numpy as np

SUB_NORMAL, SUB_UNIFORM, SUB_GAMMA_N, SUB_GAMMA_U = 0, 1, 2, 3
EDGE_RTOL = 1e-9
BINOM_CHUNK, BINOM_NMAX = 512, 1048576.0
POIS_PIECE, POIS_PIECES, POIS_STEPS = 256.0, 64, 4096
NAN = float("nan")
GAMMA_FAMILIES = ("gamma", "invgamma", "beta")
DISCRETE = ("bernoulli", "binomial", "poisson")


def pb(n):
    return 256 + n


def gb(n, e):
    return (n + 1) * 65536 + e


def _finite(*xs):
    return all(math.isfinite(x) for x in xs)


def _div(x, y):
    """IEEE x / y (Python raises on a zero divisor)."""
    if y == 0.0 and not math.isnan(x):
        return NAN if x == 0.0 else math.copysign(math.inf, x) * math.copysign(1.0, y)
    return x / y


def _near(u, cdf):
    return abs(u - cdf) <= EDGE_RTOL * abs(cdf)


def binomial(L, key, n, p, e, length):
    """key = (seed, chain, iteration, block).  Returns (count, edge)."""
    if not (0.0 <= n <= BINOM_NMAX) or n != round(n) or not (0.0 <= p <= 1.0):
        return NAN, False
    if p == 0.0:
        return 0.0, False
    if p == 1.0:
        return n, False
    flip = p > 0.5
    pp = 1.0 - p if flip else p
    q = 1.0 - pp
    s = pp / q
    l1 = L.orc_log1p(-pp)
    nt = int(n)
    C = (nt + BINOM_CHUNK - 1) // BINOM_CHUNK
    tot, edge = 0.0, False
    for c in range(C):
        nc = BINOM_CHUNK if c < C - 1 else nt - BINOM_CHUNK * (C - 1)
        u = L.orc_uniform(*key, SUB_UNIFORM, c * length + e)
        r = L.orc_exp(float(nc) * l1)
        cdf = r
        k = 0
        edge = edge or _near(u, cdf)
        while u > cdf and k < nc:
            k += 1
            r = r * (s * float(nc - k + 1) / float(k))
            cdf = cdf + r
            edge = edge or _near(u, cdf)
        tot = tot + float(nc - k if flip else k)
    return tot, edge


def poisson(L, key, lam, e, length):
    if not (lam >= 0.0) or not math.isfinite(lam):
        return NAN, False
    md = math.ceil(lam / POIS_PIECE)
    if md > POIS_PIECES:
        return NAN, False
    m = max(1, md)
    lp = lam / float(m)
    r0 = L.orc_exp(-lp)
    tot, edge = 0.0, False
    for c in range(m):
        u = L.orc_uniform(*key, SUB_UNIFORM, c * length + e)
        r = cdf = r0
        k = 0
        edge = edge or _near(u, cdf)
        while u > cdf and k < POIS_STEPS:
            k += 1
            r = r * (lp / float(k))
            cdf = cdf + r
            edge = edge or _near(u, cdf)
        tot = tot + float(k)
    return tot, edge


class _Idx:
    def __init__(self):
        self.kn = self.ku = 0


def _gamma_mt(L, key, a, ix):
    """Marsaglia & Tsang (2000), a >= 1: normals and uniforms of the block by running index."""
    d = a - 1.0 / 3.0
    c = 1.0 / math.sqrt(9.0 * d)
    while True:
        while True:
            x = L.orc_normal(*key, SUB_GAMMA_N, ix.kn)
            ix.kn += 1
            v = 1.0 + c * x
            if v > 0.0:
                break
        v = v * v * v
        u = L.orc_uniform(*key, SUB_GAMMA_U, ix.ku)
        ix.ku += 1
        x2 = x * x
        if u < 1.0 - 0.0331 * (x2 * x2):
            return d * v
        if L.orc_log(u) < 0.5 * x2 + d * (1.0 - v + L.orc_log(v)):
            return d * v


def gamma_std(L, key, a):
    """G(a), a finite and > 0, on the element block of `key`, indices from 0; a < 1 by the boost
    G(a) = G(a + 1) U^(1/a), U the next uniform after G(a + 1)'s."""
    ix = _Idx()
    if a >= 1.0:
        return _gamma_mt(L, key, a, ix)
    g = _gamma_mt(L, key, a + 1.0, ix)
    u = L.orc_uniform(*key, SUB_GAMMA_U, ix.ku)
    return g * L.orc_exp(L.orc_log(u) / a)


def sample(L, fam, a, b, seed, chain, it, n, e, length):
    """(value, edge) of element e of node n."""
    a, b = float(a), float(b)
    it = it & 0xFFFFFFFF
    key = (seed, chain, it, pb(n))
    if fam in ("normal", "isonormal"):
        if not _finite(a, b) or b < 0.0:
            return NAN, False
        return a + b * L.orc_normal(*key, SUB_NORMAL, e), False
    if fam == "bernoulli":
        if not (0.0 <= a <= 1.0):
            return NAN, False
        u = L.orc_uniform(*key, SUB_UNIFORM, e)
        return (1.0 if u < a else 0.0), _near(u, a)
    if fam == "exponential":
        if not _finite(a) or not a > 0.0:
            return NAN, False
        return -a * L.orc_log1p(-L.orc_uniform(*key, SUB_UNIFORM, e)), False
    if fam == "uniform":
        if not _finite(a, b) or b < a:
            return NAN, False
        return a + (b - a) * L.orc_uniform(*key, SUB_UNIFORM, e), False
    if fam == "binomial":
        return binomial(L, key, a, b, e, length)
    if fam == "poisson":
        return poisson(L, key, a, e, length)
    if fam in GAMMA_FAMILIES:
        if not _finite(a, b) or not a > 0.0 or not b > 0.0:
            return NAN, False
        g1 = gamma_std(L, (seed, chain, it, gb(n, e)), a)
        if fam == "gamma":
            return b * g1, False
        if fam == "invgamma":
            return _div(b, g1), False
        g2 = gamma_std(L, (seed, chain, it, gb(n, length + e)), b)
        return _div(g1, g1 + g2), False
    raise ValueError(fam)


def variates(L, fam, a, b, count, seed=1, n=0, chain0=0, it=1, length=16):
    """`count` variates of one parameter pair: elements 0 .. length - 1 of node n over successive chains."""
    out = np.empty(count)
    for q in range(count):
        out[q] = sample(L, fam, a, b, seed, chain0 + q // length, it, n, q % length, length)[0]
    return out


def widths(desc, keys):
    return [desc["nodes"][k]["len"] for k in keys]


def names(desc, keys):
    """names(m, nodekeys): y[1] ..., a scalar node by its bare name."""
    out = []
    for k in keys:
        nd = desc["nodes"][k]
        out += [k] if nd.get("scalar", False) else [f"{k}[{i + 1}]" for i in range(nd["len"])]
    return out


def predict_draws(L, value, desc, keys, seed, chain_offset=0, start=1, thin=1, rows=None):
    """(yhat rows x P x K, number of edge draws); row i has iteration start + i * thin."""
    value = np.asarray(value, float)
    n, _, K = value.shape
    i0, i1 = (0, n) if rows is None else rows
    P = sum(widths(desc, keys))
    out = np.empty((i1 - i0, P, K))
    edges = 0
    for i in range(i0, i1):
        it = start + i * thin
        for k in range(K):
            x = value[i, :, k]
            vals = {name: x[np.asarray(cols)] for name, cols in desc["cols"].items()}
            j = 0
            for key in keys:
                nd = desc["nodes"][key]
                ln = nd["len"]
                a, b = nd["params"](vals)
                a = np.broadcast_to(np.asarray(a, float), (ln,))
                b = np.broadcast_to(np.asarray(b, float), (ln,))
                for e in range(ln):
                    v, edge = sample(L, nd["fam"], a[e], b[e], seed, chain_offset + k, it, nd["id"], e, ln)
                    out[i - i0, j + e, k] = v
                    edges += bool(edge)
                j += ln
    return out, edges


def moments(yhat, shift):
    """K x P x 2: the sequential row-order sums of (yhat - shift) and its square."""
    n, P, K = yhat.shape
    acc = np.zeros((K, P, 2))
    for i in range(n):
        d = yhat[i].T - np.asarray(shift, float)[None, :]
        acc[:, :, 0] = acc[:, :, 0] + d
        acc[:, :, 1] = acc[:, :, 1] + d * d
    return acc


class FakeEngine:
    """The engine entry points predict_sharded / predict_moments_sharded use, by the restatement."""

    def __init__(self, L, value, desc, names_by_id, seed=1, chain_offset=0):
        self.L, self.value, self.desc, self.names = L, np.asarray(value, float), desc, names_by_id
        self.K, self.pmon = self.value.shape[2], self.value.shape[1]
        self.seed, self.chain_offset = seed, chain_offset
        self.calls = []
        self.h = 1   # (Chains._device_engine asks for a live handle)

    def num_kept(self):
        return self.value.shape[0]

    def _keys(self, ids):
        return [self.names[int(i)] for i in ids]

    def predict_width(self, ids):
        return sum(widths(self.desc, self._keys(ids)))

    def draws_predict(self, ids, seed, start, thin, i0=0, i1=None):
        i1 = self.num_kept() if i1 is None else i1
        self.calls.append((list(map(int, ids)), seed, start, thin, i0, i1))
        return predict_draws(self.L, self.value, self.desc, self._keys(ids), seed, self.chain_offset, start, thin,
                             (i0, i1))[0]

    def draws_predict_moments(self, ids, seed, start, thin, shift):
        return moments(self.draws_predict(ids, seed, start, thin), shift)
