"""Restatement of the ABC block update (src/samplers/abc.jl:36-144; csrc/samplers.h abc) -- the checker of ABC.

Plain Python on the oracle library's primitives only (orc_uniform, orc_normal, orc_exp, orc_log, orc_log1p,
orc_sincos2pi: the kernels' own Philox streams and elementary functions) plus IEEE arithmetic on Python floats.
One update of block b, global chain g, iteration it, with the tune row [initialised, Tsim[nsim][T],
epsilon[nsim], epsilonprime[nsim]]:

    theta0    = the block's values unlisted with transform;  logprior0 = the params' own terms at theta0
    Tobs      = the data nodes' observed summaries, concatenated
    first update (initialised == 0): Tsim[i] simulated at the current values with draw index k = 0,
              epsilon[i] = decay > 0 ? max(epsilon, d) : epsilon; otherwise the stored row
    pi0       = sum_i kernel(epsilonprime[i], d_i) * pi_error
    k = 1..maxdraw: theta1[e] = theta0[e] + scale[e] * z, z = normal #q of MMB_SUB_NORMAL or symdist(kind, q) on
              MMB_SUB_PROPOSAL, q = (k - 1) dim + e; logprior1 == -Inf skips the draw; nsim simulations at theta1;
              epsilon1[i] = (1 - decay) epsilon[i] + decay max(epsilon, min(d, epsilon[i]));
              accept iff uniform #(k - 1) of MMB_SUB_UNIFORM < pi1 / pi0 * exp(logprior1 - logprior0)

Simulated element e of data slot j, simulation i, draw k: csrc/predict_math.h's mmb_pr_elem_on restated, on the
Philox block ((b 1025 + k) 8 + i) 32 + j and the substreams MMB_SUB_ABC_N = 8 / MMB_SUB_ABC_U = 9; randeps takes
uniform #0 of slot 16.  Reductions mirror the kernel: element e on lane e % 32 in ascending e, lane partials,
then the 32-lane butterfly (partners i^1, i^2, 7 - i within 8, 15 - i within 16, i^16); min / max take lane 0.

The prior terms are the oracle's block_logpdf on a TWIN model that holds the ABC blocks' nodes alone, each block
as AMWG(params, 1.0): the same term list (the params' own terms, transform = true) and so the oracle's bits,
which the AMWG parity tests assert are the kernels' bits.  `near` counts the accept decisions whose uniform lies
within EDGE_RTOL relative of its ratio: fixtures are chosen so that it stays 0, and are then compared exactly.
"""
import ctypes as C
import math

import numpy as np

import predict_ref
import rwm_ref

SUB_NORMAL, SUB_UNIFORM, SUB_PROPOSAL, SUB_ABC_N, SUB_ABC_U = 0, 1, 5, 8, 9
MAX_DRAW, MAX_NSIM = 1024, 8
EDGE_RTOL = 1e-9
IDENTITY, SUM, MEAN, VAR, STD, MINIMUM, MAXIMUM = range(7)
NORMAL, ISONORMAL, EXPONENTIAL, UNIFORM, BINOMIAL, POISSON, BERNOULLI = 1, 2, 5, 6, 8, 9, 10
SQRT2PI = 2.50662827463100050242e+00
INF, NAN = float("inf"), float("nan")
KERNELS = ["Normal", "SymUniform", "SymTriangularDist", "Epanechnikov", "Biweight", "Triweight", "Cosine"]

PARTNERS = (lambda i: i ^ 1, lambda i: i ^ 2, lambda i: (i & ~7) | (7 - (i & 7)),
            lambda i: (i & ~15) | (15 - (i & 15)), lambda i: i ^ 16)


def abc_block(b, k, i, j):
    return ((b * (MAX_DRAW + 1) + k) * MAX_NSIM + i) * 32 + j


def _div(x, y):
    with np.errstate(all="ignore"):
        return float(np.float64(x) / np.float64(y))


def gsum(p):
    x = [float(v) for v in p]
    for f in PARTNERS:
        x = [x[i] + x[f(i)] for i in range(32)]
    return x[0]


def _gext(p, less):
    x = list(p)
    for f in PARTNERS:
        x = [x[f(i)] if (less(x[f(i)], x[i]) or x[f(i)] != x[f(i)]) else x[i] for i in range(32)]
    return x[0]


def jmax(a, b):
    if a != a:
        return a
    if b != b:
        return b
    return b if b > a else a


def jmin(a, b):
    if a != a:
        return a
    if b != b:
        return b
    return b if b < a else a


def kernel_pdf(L, kind, eps, d):
    """csrc/abc.h mmb_abc_kernel_pdf restated."""
    u = _div(d, eps)
    if kind == 0:
        return _div(L.orc_exp(-(u * u) / 2.0), eps * SQRT2PI)
    if not u <= 1.0:
        return 0.0
    w = 1.0 - u * u
    if kind == 1:
        return _div(1.0, 2.0 * eps)
    if kind == 2:
        return _div(1.0 - u, eps)
    if kind == 3:
        return _div(0.75 * w, eps)
    if kind == 4:
        return _div(0.9375 * (w * w), eps)
    if kind == 5:
        return _div(1.09375 * (w * w * w), eps)
    if kind == 6:
        s, c = C.c_double(), C.c_double()
        L.orc_sincos2pi(0.5 * u, C.byref(s), C.byref(c))
        return _div(1.0 + c.value, 2.0 * eps)
    raise ValueError(kind)


def kernel_closed_form(kind, eps, d):
    """The table of the sampler's documentation, on libm."""
    u = d / eps
    if kind == 0:
        return math.exp(-u * u / 2.0) / (eps * math.sqrt(2.0 * math.pi))
    if u > 1.0:
        return 0.0
    return {1: 1.0 / (2.0 * eps), 2: (1.0 - u) / eps, 3: 0.75 * (1.0 - u * u) / eps,
            4: 15.0 / 16.0 * (1.0 - u * u) ** 2 / eps, 5: 35.0 / 32.0 * (1.0 - u * u) ** 3 / eps,
            6: (1.0 + math.cos(math.pi * u)) / (2.0 * eps)}[kind]


def exp_pdf(L, eps, x):
    return _div(L.orc_exp(_div(-x, eps)), eps)


class _AbcStreams:
    """The oracle library with predict_ref's substreams moved to ABC's: normal 0 -> 8, uniform 1 -> 9."""

    def __init__(self, L):
        self.L = L

    def __getattr__(self, name):
        return getattr(self.L, name)

    def orc_uniform(self, seed, chain, it, block, sub, k):
        return self.L.orc_uniform(seed, chain, it, block, SUB_ABC_U if sub == SUB_UNIFORM else sub, k)

    def orc_normal(self, seed, chain, it, block, sub, k):
        return self.L.orc_normal(seed, chain, it, block, SUB_ABC_N if sub == SUB_NORMAL else sub, k)


def draw(L, fam, a, b, key, e, length):
    """csrc/predict_math.h mmb_pr_elem_on restated; key = (seed, chain, iteration, block)."""
    a, b = float(a), float(b)
    if fam in (NORMAL, ISONORMAL):
        if not (math.isfinite(a) and math.isfinite(b)) or b < 0.0:
            return NAN
        return a + b * L.orc_normal(*key, SUB_ABC_N, e)
    if fam == BERNOULLI:
        if not 0.0 <= a <= 1.0:
            return NAN
        return 1.0 if L.orc_uniform(*key, SUB_ABC_U, e) < a else 0.0
    if fam == EXPONENTIAL:
        if not math.isfinite(a) or not a > 0.0:
            return NAN
        return -a * L.orc_log1p(-L.orc_uniform(*key, SUB_ABC_U, e))
    if fam == UNIFORM:
        if not (math.isfinite(a) and math.isfinite(b)) or b < a:
            return NAN
        return a + (b - a) * L.orc_uniform(*key, SUB_ABC_U, e)
    if fam == BINOMIAL:
        return predict_ref.binomial(_AbcStreams(L), key, a, b, e, length)[0]
    if fam == POISSON:
        return predict_ref.poisson(_AbcStreams(L), key, a, e, length)[0]
    raise ValueError(fam)


def summarise(x, codes):
    """One node's summary of its elements x (floats), by the kernel's reduction order."""
    n = len(x)
    if codes[0] == IDENTITY:
        return list(x)
    ps, lo, hi = [0.0] * 32, [INF] * 32, [-INF] * 32
    for e in range(n):
        ln, xe = e % 32, x[e]
        ps[ln] = ps[ln] + xe
        lo[ln] = xe if (xe < lo[ln] or xe != xe) else lo[ln]
        hi[ln] = xe if (xe > hi[ln] or xe != xe) else hi[ln]
    total = gsum(ps)
    mean = _div(total, float(n))
    var = 0.0
    if VAR in codes or STD in codes:
        pq = [0.0] * 32
        for e in range(n):
            dv = x[e] - mean
            pq[e % 32] = pq[e % 32] + dv * dv
        var = _div(gsum(pq), float(n - 1))
    mn = _gext(lo, lambda p, q: p < q)
    mx = _gext(hi, lambda p, q: p > q)
    pick = {SUM: total, MEAN: mean, VAR: var, STD: math.sqrt(var) if var == var and var >= 0.0 else NAN,
            MINIMUM: mn, MAXIMUM: mx}
    return [pick[c] for c in codes]


def dist(ts, tobs):
    sq = [0.0] * 32
    for t in range(len(ts)):
        df = ts[t] - tobs[t]
        sq[t] = df * df
    s = gsum(sq)
    return math.sqrt(s) if s == s else NAN


class Data:
    """One data node: `params(vals) -> (a, b)` in Distributions order, scalars or arrays of `length`, evaluated
    with the operations of the node's expression on vals[name] (numpy float64 arrays of the state and inputs)."""

    def __init__(self, name, fam, length, params):
        self.name, self.fam, self.length, self.params = name, fam, length, params


class TwinPrior:
    """logpdf(model, params, true) of the ABC blocks by the oracle's block_logpdf on `twin`: a model of the ABC
    blocks' nodes alone whose block `tb[b]` is AMWG(params of block b, 1.0)."""

    def __init__(self, oracle, model, twin, tb):
        self.o, self.m, self.twin, self.tb = oracle, model, twin, dict(tb)
        oracle._ir(twin)
        self.spec = twin.spec()
        self.arrs, self.ptrs, self.ns = oracle._data(twin)
        self.map = [(tn.offset, model.nodes[name].offset, tn.dim) for name, tn in twin.nodes.items()]

    def __call__(self, b, row, x):
        dp = C.POINTER(C.c_double)
        tw = np.zeros(self.twin.nvalues)
        for to, mo, dim in self.map:
            tw[to:to + dim] = row[mo:mo + dim]
        self.o._ir(self.twin)
        xx = np.ascontiguousarray(x, dtype=np.float64)
        return self.o.L.orc_block_logpdf(C.byref(self.spec), self.ptrs, self.ns, tw.ctypes.data_as(dp), self.tb[b],
                                         xx.ctypes.data_as(dp))


class Restatement:
    """ABC updates of `model` (a lowered ir.Model) on canonical value rows.  `data[name]`: the Data of every data
    node; `prior(b, row, x)`: the params' own log density at the transformed x (TwinPrior)."""

    def __init__(self, L, mb, model, data, prior, seed, chain_offset=0):
        self.L, self.mb, self.m, self.prior = L, mb, model, prior
        self.seed, self.off = int(seed), int(chain_offset)
        a = mb.abi
        self.blocks = {}
        for b, s in enumerate(model.samplers):
            if s.kind != a.MMB_SAMPLER_ABC:
                continue
            idx, pos = [], []
            for p in s.params:
                n = model.nodes[p]
                fam = model.traced[p].fam
                lk = (1 if n.positive else 0, 0.0, 0.0)
                if fam == a.MMB_IR_BETA:
                    lk = (2, 0.0, 0.0)
                elif fam == a.MMB_IR_UNIFORM:
                    N = model.ir().nodes[n.id]
                    lk = (3, float(N.lo), float(N.hi))
                idx += list(range(n.offset, n.offset + n.dim))
                pos += [lk] * n.dim
            sc = s.spec_tuning(len(idx))[:len(idx)]
            self.blocks[b] = (s, idx, pos, [float(v) for v in sc], [data[nm] for nm in s.abc_data])
        self.updates = {b: 0 for b in self.blocks}
        self.accepts = {b: 0 for b in self.blocks}
        self.skipped = {b: 0 for b in self.blocks}   # draws skipped at logprior1 == -Inf
        self.near = 0

    def tune_len(self, b):
        s = self.blocks[b][0]
        return 1 + s.nsim * (s.abc_T + 2)

    def tune0(self, K):
        return {b: np.zeros((K, self.tune_len(b))) for b in self.blocks}

    def vals_of(self, row):
        m = self.m
        v = {k: np.asarray(x, dtype=np.float64) for k, x in m.inputs.items()}
        for name, n in m.nodes.items():
            v[name] = np.array(row[n.offset:n.offset + n.dim], dtype=np.float64)
        for name in m.fixed:
            v[name] = np.asarray(m.fixed_vals[name], dtype=np.float64)
        return v

    def stats(self, b, vals, key):
        """The concatenated summaries: observed (key None) or simulated for key = (chain, it, k, i)."""
        s, _, _, _, data = self.blocks[b]
        out = []
        for j, dn in enumerate(data):
            if key is None:
                x = [float(t) for t in vals[dn.name]]
            else:
                g, it, k, i = key
                with np.errstate(all="ignore"):
                    pa, pb = dn.params(vals)
                pa = np.broadcast_to(np.asarray(pa, dtype=np.float64), (dn.length,))
                pb = np.broadcast_to(np.asarray(pb, dtype=np.float64), (dn.length,))
                pk = (self.seed, g, it, abc_block(b, k, i, j))
                x = [draw(self.L, dn.fam, pa[e], pb[e], pk, e, dn.length) for e in range(dn.length)]
            out += summarise(x, s.abc_codes)
        assert len(out) == s.abc_T
        return out

    def _tolerance(self, b, g, it, k, i, ei, randeps):
        if not randeps:
            return ei, 1.0
        u = self.L.orc_uniform(self.seed, g, it, abc_block(b, k, i, 16), SUB_ABC_U, 0)
        epi = -ei * self.L.orc_log1p(-u)
        return epi, exp_pdf(self.L, ei, epi)

    def update(self, row, b, chain, it, tune):
        """One ABC update of block b on the value row and its tune row (both in place); whether it accepted."""
        s, idx, pos, scale, _ = self.blocks[b]
        L, d, T, nsim = self.L, len(idx), s.abc_T, s.nsim
        g, it32 = self.off + chain, it & 0xFFFFFFFF
        eps, decay = float(s.epsilon), float(s.decay)
        v = [rwm_ref.link(L, p[0], row[i], p[1], p[2]) for i, p in zip(idx, pos)]
        lp0 = self.prior(b, row, v)
        tobs = self.stats(b, self.vals_of(row), None)
        first = tune[0] == 0.0
        pi0, e0 = 0.0, [0.0] * nsim
        for i in range(nsim):
            if first:
                ts = self.stats(b, self.vals_of(row), (g, it32, 0, i))
                dd = dist(ts, tobs)
                ei = jmax(eps, dd) if decay > 0.0 else eps
                epi, perr = self._tolerance(b, g, it32, 0, i, ei, s.randeps)
                tune[1 + i * T:1 + (i + 1) * T] = ts
                tune[1 + nsim * T + i] = ei
                tune[1 + nsim * T + nsim + i] = epi
            else:
                ts = [float(t) for t in tune[1 + i * T:1 + (i + 1) * T]]
                ei, epi = float(tune[1 + nsim * T + i]), float(tune[1 + nsim * T + nsim + i])
                dd = dist(ts, tobs)
                perr = exp_pdf(L, ei, epi) if s.randeps else 1.0
            pi0 = pi0 + kernel_pdf(L, s.kernel, epi, dd) * perr
            e0[i] = ei
        acc = False
        x = v
        for k in range(1, s.maxdraw + 1):
            x = []
            for e in range(d):
                q = (k - 1) * d + e
                z = (L.orc_normal(self.seed, g, it32, b, SUB_NORMAL, q) if s.proposal == 0
                     else rwm_ref.symdist(L, s.proposal, self.seed, g, it32, b, q))
                x.append(v[e] + scale[e] * z)
            lp1 = self.prior(b, row, x)
            if lp1 == -INF:
                self.skipped[b] += 1
                continue
            cand = np.array(row, dtype=np.float64)
            for q, (i, p) in enumerate(zip(idx, pos)):
                cand[i] = rwm_ref.invlink(L, p[0], x[q], p[1], p[2])
            cvals = self.vals_of(cand)
            pi1, ts1, e1, ep1 = 0.0, [], [], []
            for i in range(nsim):
                ts = self.stats(b, cvals, (g, it32, k, i))
                dd = dist(ts, tobs)
                ei = (1.0 - decay) * e0[i] + decay * jmax(eps, jmin(dd, e0[i]))
                epi, perr = self._tolerance(b, g, it32, k, i, ei, s.randeps)
                pi1 = pi1 + kernel_pdf(L, s.kernel, epi, dd) * perr
                ts1.append(ts)
                e1.append(ei)
                ep1.append(epi)
            u = L.orc_uniform(self.seed, g, it32, b, SUB_UNIFORM, k - 1)
            with np.errstate(all="ignore"):
                ratio = float(np.float64(_div(pi1, pi0)) * np.float64(L.orc_exp(lp1 - lp0)))
            if math.isfinite(ratio) and abs(u - ratio) <= EDGE_RTOL * abs(ratio):
                self.near += 1
            if u < ratio:
                acc = True
                for i in range(nsim):
                    tune[1 + i * T:1 + (i + 1) * T] = ts1[i]
                    tune[1 + nsim * T + i] = e1[i]
                    tune[1 + nsim * T + nsim + i] = ep1[i]
                break
        tune[0] = 1.0
        w = x if acc else v
        for q, (i, p) in enumerate(zip(idx, pos)):
            row[i] = rwm_ref.invlink(L, p[0], w[q], p[1], p[2])
        self.updates[b] += 1
        self.accepts[b] += int(acc)
        return acc

    def monitored(self, row):
        m = self.m
        col = {}
        for n in m.nodes.values():
            for i in range(n.dim):
                col[f"{n.name}[{i + 1}]"] = row[n.offset + i]
            if n.dim == 1:
                col[n.name] = row[n.offset]
        return [col[name] for name in m.monitor_names]

    def run(self, values, iters, burnin=0, thin=1, tunes=None, it0=0):
        """Sweeps of a scheme whose blocks are all ABC, on values [K, P] and tunes {b: [K, L]} in place.  Returns
        the kept draws [n, p, K] (Chains order), or None."""
        K = values.shape[0]
        assert len(self.blocks) == len(self.m.samplers), "the restatement sweeps ABC blocks only"
        kept = []
        for it in range(it0 + 1, it0 + iters + 1):
            for c in range(K):
                for b in sorted(self.blocks):
                    self.update(values[c], b, c, it, tunes[b][c])
            if it > burnin and (it - burnin) % thin == 0:
                kept.append([self.monitored(values[c]) for c in range(K)])
        if not kept:
            return None
        return np.asfortranarray(np.transpose(np.array(kept), (0, 2, 1)))

    def replay(self, b, init, draws, tune, it0=0):
        """Block b's updates replayed from the device's own pre-update rows, for a scheme whose block 0 is the ABC
        block b and whose every node is monitored in state order: draws [n, P, K] (thin 1, no burn-in), init
        [K, P].  `tune` [K, L] is carried in place.  Returns the number of rows whose block values differ."""
        n, _, K = draws.shape
        _, idx, _, _, _ = self.blocks[b]
        bad = 0
        for c in range(K):
            for t in range(n):
                row = np.array(init[c] if t == 0 else draws[t - 1, :, c], dtype=np.float64)
                self.update(row, b, c, it0 + t + 1, tune[c])
                bad += int(not np.array_equal(row[idx], draws[t, idx, c]))
        return bad

    def stats_counts(self):
        return {b: {"updates": self.updates[b], "accepts": self.accepts[b]} for b in self.blocks}

    def tune(self, tunes):
        return np.concatenate([tunes[b] for b in sorted(tunes)], axis=1)


# ------------------------------------------------------------------ fixtures shared by test_abc.py and test_gpu_abc.py
# make(mb, K) -> (model with its scheme set, init matrix [K, P], {data node: Data}, twin model, {ABC block: twin block})

def _finish(mb, m, tw, inits, tw_keys, data, scheme, K):
    m.setsamplers(scheme)
    V = m.init_matrix(inits, K)
    abc = [b for b, s in enumerate(scheme) if s.kind == mb.abi.MMB_SAMPLER_ABC]
    tw.setsamplers([mb.AMWG(list(scheme[b].params), 1.0) for b in abc])
    tw.init_matrix([{k: d[k] for k in tw_keys} for d in inits], K)
    return m, V, data, tw, {b: i for i, b in enumerate(abc)}


def line_abc(mb, K, scheme=None, seed=1):
    """doc/examples/line_abc.jl (ir.line_abc_model); the default scheme is the published one with maxdraw = 4."""
    ir = mb.ir
    m = ir.line_abc_model().setinputs(ir.line_abc_inputs())
    tw = ir.Model(beta=ir.Stochastic(1, lambda: ir.MvNormal(2, math.sqrt(100))),
                  s2=ir.Stochastic(lambda: ir.InverseGamma(0.01, 0.01)))
    data = {"y": Data("y", ISONORMAL, 5, lambda v: (v["beta"][0] + v["beta"][1] * v["x"], np.sqrt(v["s2"][0])))}
    scheme = ir.line_abc_scheme(maxdraw=4) if scheme is None else scheme
    return _finish(mb, m, tw, ir.line_abc_inits(K, seed), ("beta", "s2"), data, scheme, K)


def kernel_scheme(mb, i, **kw):
    """Kernel i on both line_abc blocks, with proposals i + 3 and i + 4 (mod 7): over i = 0..6 all seven appear."""
    kw = {"maxdraw": 3, "nsim": 2, "decay": 0.75, **kw}  # (decay < 1 keeps the distances inside the kernels' supports)
    return [mb.ABC("beta", [0.5, 0.25], "identity", 2.0, kernel=KERNELS[i], proposal=KERNELS[(i + 3) % 7], **kw),
            mb.ABC("s2", 0.5, ("mean", "std"), 0.5, kernel=KERNELS[i], proposal=KERNELS[(i + 4) % 7], **kw)]


def caps(mb, K):
    """nsim = 8 with T = 32: one Normal data node of 32 elements, identity."""
    ir = mb.ir
    rng = np.random.default_rng(3)
    y = list(np.round(rng.normal(0.5, 1.0, 32), 3))
    m = ir.Model(y=ir.Stochastic(1, lambda mu: ir.Normal(mu, 1.0), False), mu=ir.Stochastic(lambda: ir.Normal(0.0, 10.0)))
    tw = ir.Model(mu=ir.Stochastic(lambda: ir.Normal(0.0, 10.0)))
    inits = [{"y": y, "mu": float(rng.normal())} for _ in range(K)]
    data = {"y": Data("y", NORMAL, 32, lambda v: (v["mu"][0], 1.0))}
    scheme = [mb.ABC("mu", 0.3, "identity", 4.0, kernel="Biweight", maxdraw=3, nsim=8, decay=0.5)]
    return _finish(mb, m, tw, inits, ("mu",), data, scheme, K)


def wide(mb, K):
    """A Normal data node of 70 elements under all six statistics: strided lanes, a ragged last pass; a block of
    two nodes."""
    ir = mb.ir
    rng = np.random.default_rng(4)
    y = list(np.round(rng.normal(1.0, 2.0, 70), 3))
    m = ir.Model(y=ir.Stochastic(1, lambda mu, s2: ir.Normal(mu, ir.sqrt(s2)), False),
                 mu=ir.Stochastic(lambda: ir.Normal(0.0, 10.0)), s2=ir.Stochastic(lambda: ir.InverseGamma(2.0, 2.0)))
    tw = ir.Model(mu=ir.Stochastic(lambda: ir.Normal(0.0, 10.0)), s2=ir.Stochastic(lambda: ir.InverseGamma(2.0, 2.0)))
    inits = [{"y": y, "mu": float(rng.normal()), "s2": float(rng.gamma(2.0))} for _ in range(K)]
    data = {"y": Data("y", NORMAL, 70, lambda v: (v["mu"][0], np.sqrt(v["s2"][0])))}
    scheme = [mb.ABC(["mu", "s2"], [0.3, 0.2], ("sum", "mean", "var", "std", "minimum", "maximum"), 3.0,
                     kernel="SymTriangularDist", maxdraw=3, nsim=2, decay=0.75)]
    return _finish(mb, m, tw, inits, ("mu", "s2"), data, scheme, K)


def families(mb, K):
    """Bernoulli, Binomial, Poisson, Exponential and Uniform data nodes, 3 elements each, identity: T = 15."""
    ir = mb.ir
    rng = np.random.default_rng(5)
    m = ir.Model(yb=ir.Stochastic(1, lambda p: ir.Bernoulli(p), False),
                 yn=ir.Stochastic(1, lambda n, p: ir.Binomial(n, p), False),
                 yp=ir.Stochastic(1, lambda lam, t: ir.Poisson(lam * t), False),
                 ye=ir.Stochastic(1, lambda lam: ir.Exponential(lam), False),
                 yu=ir.Stochastic(1, lambda lam, w: ir.Uniform(0.0, lam * w), False),
                 p=ir.Stochastic(lambda: ir.Beta(2.0, 3.0)), lam=ir.Stochastic(lambda: ir.Exponential(2.0)))
    m.setinputs({"n": [5.0, 10.0, 20.0], "t": [1.0, 2.0, 300.0], "w": [1.0, 2.0, 3.0]})
    tw = ir.Model(p=ir.Stochastic(lambda: ir.Beta(2.0, 3.0)), lam=ir.Stochastic(lambda: ir.Exponential(2.0)))
    obs = {"yb": [1.0, 0.0, 1.0], "yn": [2.0, 4.0, 9.0], "yp": [1.0, 3.0, 400.0], "ye": [0.7, 1.9, 0.4],
           "yu": [0.5, 1.0, 2.5]}
    inits = [{**obs, "p": float(rng.uniform(0.2, 0.8)), "lam": float(rng.uniform(0.8, 2.5))} for _ in range(K)]
    data = {"yb": Data("yb", BERNOULLI, 3, lambda v: (v["p"][0], 0.0)),
            "yn": Data("yn", BINOMIAL, 3, lambda v: (v["n"], v["p"][0])),
            "yp": Data("yp", POISSON, 3, lambda v: (v["lam"][0] * v["t"], 0.0)),
            "ye": Data("ye", EXPONENTIAL, 3, lambda v: (v["lam"][0], 0.0)),
            "yu": Data("yu", UNIFORM, 3, lambda v: (0.0, v["lam"][0] * v["w"]))}
    scheme = [mb.ABC(["p", "lam"], [0.4, 0.3], "identity", 30.0, kernel="Cosine", proposal="SymUniform", maxdraw=3,
                     nsim=2)]
    return _finish(mb, m, tw, inits, ("p", "lam"), data, scheme, K)


def hierarchical(mb, K):
    """The data node theta is itself sampled, by an AMWG block after the ABC block: Tobs moves between iterations."""
    ir = mb.ir
    rng = np.random.default_rng(6)
    m = ir.Model(y=ir.Stochastic(1, lambda theta: ir.Normal(theta, 0.5), False),
                 mu=ir.Stochastic(lambda: ir.Normal(0.0, 10.0)),
                 theta=ir.Stochastic(1, lambda mu: ir.Normal(mu, 1.0)))
    tw = ir.Model(mu=ir.Stochastic(lambda: ir.Normal(0.0, 10.0)))
    inits = [{"y": [0.3, 1.1, -0.4, 0.9], "mu": float(rng.normal()), "theta": rng.normal(0.5, 1.0, 4)} for _ in range(K)]
    data = {"theta": Data("theta", NORMAL, 4, lambda v: (v["mu"][0], 1.0))}
    scheme = [mb.ABC("mu", 0.5, ("mean", "maximum"), 0.3, kernel="Normal", maxdraw=3, nsim=2, decay=0.75),
              mb.AMWG("theta", 1.0)]
    return _finish(mb, m, tw, inits, ("mu",), data, scheme, K)


def beta_binomial(mb, K, nsim=2, seed=7):
    """p ~ Beta(2, 3), y ~ Binomial(10, p), y = 3: with identity, SymUniform and epsilon < 1 the ABC target is
    the exact posterior Beta(5, 10)."""
    ir = mb.ir
    rng = np.random.default_rng(seed)
    m = ir.Model(y=ir.Stochastic(1, lambda n, p: ir.Binomial(n, p), False), p=ir.Stochastic(lambda: ir.Beta(2.0, 3.0)))
    m.setinputs({"n": [10.0]})
    tw = ir.Model(p=ir.Stochastic(lambda: ir.Beta(2.0, 3.0)))
    inits = [{"y": [3.0], "p": float(rng.beta(2.0, 3.0))} for _ in range(K)]
    data = {"y": Data("y", BINOMIAL, 1, lambda v: (v["n"], v["p"][0]))}
    scheme = [mb.ABC("p", 1.0, "identity", 0.5, kernel="SymUniform", maxdraw=1, nsim=nsim, decay=1.0)]
    return _finish(mb, m, tw, inits, ("p",), data, scheme, K)


def beta_bernoulli(mb, K, seed=8):
    """p ~ Beta(2, 3), y[8] ~ Bernoulli(p) with three ones, "sum": the exact posterior is Beta(5, 8)."""
    ir = mb.ir
    rng = np.random.default_rng(seed)
    m = ir.Model(y=ir.Stochastic(1, lambda p: ir.Bernoulli(p), False), p=ir.Stochastic(lambda: ir.Beta(2.0, 3.0)))
    tw = ir.Model(p=ir.Stochastic(lambda: ir.Beta(2.0, 3.0)))
    inits = [{"y": [1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0], "p": float(rng.beta(2.0, 3.0))} for _ in range(K)]
    data = {"y": Data("y", BERNOULLI, 8, lambda v: (v["p"][0], 0.0))}
    scheme = [mb.ABC("p", 1.0, "sum", 0.5, kernel="SymUniform", maxdraw=1, nsim=1, decay=1.0)]
    return _finish(mb, m, tw, inits, ("p",), data, scheme, K)


def restatement(oracle, mb, made, seed, chain_offset=0):
    m, V, data, tw, tb = made
    return Restatement(oracle.L, mb, m, data, TwinPrior(oracle, m, tw, tb), seed, chain_offset)


def restate(oracle, mb, made, seed, iters, burnin=0, thin=1):
    """A whole all-ABC run restated: (draws, final values, tune rows, counts, near, skipped)."""
    R = restatement(oracle, mb, made, seed)
    vals = made[1].copy()
    tunes = R.tune0(vals.shape[0])
    d = R.run(vals, iters, burnin=burnin, thin=thin, tunes=tunes)
    return d, vals, R.tune(tunes), R.stats_counts(), R.near, sum(R.skipped.values())
