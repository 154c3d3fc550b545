"""BMG, BMC3 and BIA (src/samplers/bmg.jl:57-101, bmc3.jl:57-65, bia.jl:70-119) restated in plain Python: the
checker of tests/test_gpu_binary.py, in the style of tests/dgs_ref.py.

    index set   int k: a partial Fisher-Yates shuffle of 0..n-1, for j = 0..k-1 swap positions j and
                r = j + min(floor(u_j (n - j)), n - j - 1), u_j = uniform #j of the block's SUB_BINARY stream; the set
                is the first k positions.  Lists: list number min(floor(u_0 m), m - 1) of the m lists.
    BMC3        x = v with the set's elements flipped; accepted iff u < exp(logf(x) - logf(v)), u = uniform #0 of
                SUB_UNIFORM
    BMG         p_i = invlogit(logf(x | x_i = 1) - logf(x | x_i = 0)) for i in the set, 0.5 unless 0 < p_i < 1;
                theta_i = (uniform #(1 + i) of SUB_UNIFORM < p_i); y = x with theta; qy, qx summed over the set in
                ascending order; accepted iff u < exp((logf(y) - qy) - (logf(x) - qx)); n = 1: theta is the value
    BIA         element j moves iff uniform #j of SUB_BINARY < A_j (a 0) or D_j (a 1); q_ratio over j ascending;
                alpha = min(1, exp(logf(x) - logf(v)) q_ratio); A, D adapt (bia.jl:101-111) with
                iter^(-decay) = exp(-decay log(iter)); accepted iff uniform #0 of SUB_UNIFORM < alpha; a NaN alpha
                rejects and leaves the tune row as it was

The log densities are the test models' own formulas written out with math.log / math.lgamma / math.fsum; no project
code except `orc_uniform` of the oracle library.  It is a reference, not a copy of the device's summation order,
so the comparison is decision-exact away from thresholds: a comparison u < t is "near" when |u - t| <= DELTA,
the DELTA and the reasoning of dgs_ref.py (absolute log-density terms sum to at most 1e4, so a rounded sum is
within about 1e-10 of exact).  The compared values are the accept ratio (near only where the ratio is at most
1 + DELTA, since u < 1), a BMG p_i and a BIA A_j or D_j.  At a near comparison the device may decide either
way: the replay explores both, adopts the device's result if some path gives it, and counts a skip.
"""
import inspect
import math

import numpy as np

from dgs_ref import DELTA, normal_lp

SUB_UNIFORM, SUB_BINARY = 1, 7


def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def invlogit(x):
    return 1.0 / (_exp(-x) + 1.0)


def index_set(u, n, k):
    """The ascending 0-based index set; u(j) = uniform #j of the block's SUB_BINARY stream."""
    if isinstance(k, int):
        perm = list(range(n))
        for j in range(k):
            r = j + min(int(math.floor(u(j) * (n - j))), n - j - 1)
            perm[j], perm[r] = perm[r], perm[j]
        return sorted(perm[:k])
    q = min(int(math.floor(u(0) * len(k))), len(k) - 1)
    return sorted({i - 1 for i in k[q]})


class Dec:
    """The threshold comparisons of one update: lt(u, t) is u < t, and where |u - t| <= DELTA the choice is a
    recorded branch point that `forced` may override."""

    def __init__(self, forced=()):
        self.forced, self.nears = forced, []

    def lt(self, u, t):
        natural = u < t
        if not abs(u - t) <= DELTA:
            return natural
        i = len(self.nears)
        self.nears.append(self.forced[i] if i < len(self.forced) else natural)
        return self.nears[i]


def explore(step, forced=()):
    """[primary outcome, alternatives...] of step(Dec): every combination of choices at near comparisons."""
    d = Dec(forced)
    outs = [step(d)]
    for i in range(len(forced), len(d.nears)):
        outs += explore(step, tuple(d.nears[:i]) + (not d.nears[i],))
    return outs


class BNode:
    """One binary block: the node's name and length, logf(st) -> logpdf!(block, st[name]) and the sampler:
    kind "bmg" | "bmc3" (k) or "bia" (epsilon, decay, target)."""

    def __init__(self, name, n, logf, kind, k=1, epsilon=None, decay=0.55, target=0.45):
        self.name, self.n, self._logf, self.kind, self.k = name, n, logf, kind, k
        self.epsilon = 0.01 / n if epsilon is None else epsilon
        self.decay, self.target = decay, target
        self.evals = 0
        self.halves = 0  # BMG: p_i replaced by 0.5

    def logf(self, st, x):
        self.evals += 1
        old = st[self.name]
        st[self.name] = list(x)
        try:
            return self._logf(st)
        finally:
            st[self.name] = old


def bmc3_step(node, st, ub, uu, dec):
    """-> (new value, accepted)"""
    v = list(st[node.name])
    x = list(v)
    for i in index_set(ub, node.n, node.k):
        x[i] = 1.0 - v[i]
    ratio = _exp(node.logf(st, x) - node.logf(st, v))
    acc = dec.lt(uu(0), ratio)
    return (x if acc else v), acc


def _pbernoulli(node, st, x, lf, idx, probs):
    for i in idx:
        y = list(x)
        y[i] = 1.0 - x[i]
        lo = node.logf(st, y)
        p = invlogit(lf - lo if x[i] == 1.0 else lo - lf)
        if not 0.0 < p < 1.0:
            p = 0.5
            node.halves += 1
        probs[i] = p


def bmg_step(node, st, ub, uu, dec):
    v = list(st[node.name])
    idx = index_set(ub, node.n, node.k)
    probs = [0.5] * node.n
    lfx = node.logf(st, v)
    _pbernoulli(node, st, v, lfx, idx, probs)
    y = list(v)
    for i in idx:
        y[i] = 1.0 if dec.lt(uu(1 + i), probs[i]) else 0.0
    if node.n == 1:
        return y, True
    qy = 0.0
    for i in idx:
        qy = qy + (math.log(probs[i]) if y[i] == 1.0 else math.log(1.0 - probs[i]))
    lfy = node.logf(st, y)
    _pbernoulli(node, st, y, lfy, idx, probs)
    qx = 0.0
    for i in idx:
        qx = qx + (math.log(probs[i]) if v[i] == 1.0 else math.log(1.0 - probs[i]))
    acc = dec.lt(uu(0), _exp((lfy - qy) - (lfx - qx)))
    return (y if acc else v), acc


def bia_step(node, st, tune, ub, uu, dec):
    """tune = [iter, A[n], D[n]] -> (new value, accepted, new tune row)"""
    n, eps = node.n, node.epsilon
    it, A, D = int(tune[0]) + 1, list(tune[1:1 + n]), list(tune[1 + n:1 + 2 * n])
    v = list(st[node.name])
    x, added, deleted, q = list(v), [0.0] * n, [0.0] * n, 1.0
    for j in range(n):
        if v[j] == 0.0:
            if dec.lt(ub(j), A[j]):
                x[j], added[j] = 1.0, 1.0
                q = q * (D[j] / A[j])
        elif dec.lt(ub(j), D[j]):
            x[j], deleted[j] = 0.0, 1.0
            q = q * (A[j] / D[j])
    r = _exp(node.logf(st, x) - node.logf(st, v)) * q
    if r != r:
        return v, False, list(tune)
    alpha = min(1.0, r)
    g = math.exp(-node.decay * math.log(it))
    for j in range(n):
        c = math.log((A[j] - eps) / (1.0 - A[j] - eps)) + g * added[j] * (alpha - node.target)
        A[j] = (math.exp(c) * (1.0 - eps) + eps) / (1.0 + math.exp(c))
        c = math.log((D[j] - eps) / (1.0 - D[j] - eps)) + g * deleted[j] * (alpha - node.target)
        D[j] = (math.exp(c) * (1.0 - eps) + eps) / (1.0 + math.exp(c))
    acc = dec.lt(uu(0), alpha)
    return (x if acc else v), acc, [float(it)] + A + D


class Spec:
    """blocks: the scheme in device block order, each ("bin", BNode) or ("other", [node names])."""

    def __init__(self, blocks, columns):
        self.blocks, self.columns = blocks, columns


class Replay:
    """Replays chains from their inits update by update against the device's draws (thin 1, burnin 0, every
    sampled node monitored): draws[t, column, chain].  BIA blocks take `tunes`: the device's tune rows
    [window][chain][row] read before the first and after every iteration (one iteration per window)."""

    def __init__(self, orc_uniform, spec, seed, chain_offset=0):
        self.u, self.spec, self.seed, self.off = orc_uniform, spec, seed, chain_offset
        self.skips = self.updates = self.accepts = 0
        self.mismatch = []
        self.tune_err = 0.0

    def state(self, row):
        return {n: [float(x) for x in row[c0:c0 + ln]] for n, (c0, ln) in self.spec.columns.items()}

    def streams(self, c, it, b):
        return (lambda j: self.u(self.seed, self.off + c, it, b, SUB_BINARY, j),
                lambda j: self.u(self.seed, self.off + c, it, b, SUB_UNIFORM, j))

    def step(self, node, st, c, it, b, tune=None):
        ub, uu = self.streams(c, it, b)
        if node.kind == "bia":
            return explore(lambda d: bia_step(node, st, tune, ub, uu, d))
        fn = bmg_step if node.kind == "bmg" else bmc3_step
        return explore(lambda d: fn(node, st, ub, uu, d))

    def chain(self, c, init_row, draws, it0=0, tunes=None):
        st = self.state(init_row)
        for t in range(draws.shape[0]):
            dev = self.state(draws[t, :, c])
            for b, (kind, what) in enumerate(self.spec.blocks):
                if kind != "bin":  # another sampler's block: its new values are the draw's
                    for n in what:
                        st[n] = list(dev[n])
                    continue
                self.updates += 1
                got = dev[what.name]
                outs = self.step(what, st, c, it0 + t + 1, b, None if tunes is None else tunes[t][c])
                hit = next((o for o in outs if o[0] == got), None)
                if hit is None:
                    self.mismatch.append((c, it0 + t + 1, what.name, got, outs[0][0]))
                    hit = outs[0]
                elif hit is not outs[0]:
                    self.skips += 1
                self.accepts += bool(hit[1])
                if tunes is not None and hit is outs[0]:
                    want, have = hit[2], tunes[t + 1][c]
                    if want[0] != have[0]:
                        self.mismatch.append((c, it0 + t + 1, "iter", have[0], want[0]))
                    for w, h in zip(want[1:], have[1:]):
                        self.tune_err = max(self.tune_err, abs(w - h) / abs(w))
                st[what.name] = list(got)  # continue from the device's state
        return st

    def run(self, init, draws, it0=0, tunes=None):
        for c in range(draws.shape[2]):
            self.chain(c, init[c], draws, it0, tunes)
        return self


def forward(orc_uniform, spec, seed, init_row, chain, iters):
    """The restatement alone (binary-only schemes): (draw rows, thresholds met), BIA from its initial tune row."""
    R = Replay(orc_uniform, spec, seed)
    st = R.state(init_row)
    near, rows = 0, []
    tune = {b: [0.0] + [1.0 / nd.n] * (2 * nd.n) for b, (k, nd) in enumerate(spec.blocks) if k == "bin"}
    for t in range(iters):
        for b, (kind, node) in enumerate(spec.blocks):
            assert kind == "bin"
            ub, uu = R.streams(chain, t + 1, b)
            d = Dec()
            if node.kind == "bia":
                st[node.name], _, tune[b] = bia_step(node, st, tune[b], ub, uu, d)
            else:
                st[node.name], _ = (bmg_step if node.kind == "bmg" else bmc3_step)(node, st, ub, uu, d)
            near += len(d.nears)
        row = [0.0] * sum(ln for _, ln in spec.columns.values())
        for n, (c0, ln) in spec.columns.items():
            row[c0:c0 + ln] = st[n]
        rows.append(row)
    return rows, near


# ------------------------------------------------------------------ the test models
# Variable selection with fixed coefficients, as in doc/samplers/bmg.jl: y_i ~ Normal(sum_j x_ij beta0_j gamma_j, 1),
# 25 observations, gamma ~ Bernoulli(0.5) (or DiscreteUniform(0, 1)); data from a fixed numpy RandomState.

NOBS = 25


class Data:
    def __init__(self, n, seed, coef, active, scale=None):
        rs = np.random.RandomState(seed)
        X = rs.standard_normal((NOBS, n))
        if scale is not None:
            X = X * np.asarray(scale, dtype=float)
        self.n = n
        self.b0 = [float(coef[j % len(coef)]) for j in range(n)]
        truth = np.array([self.b0[j] if j in active else 0.0 for j in range(n)])
        self.y = [float(v) for v in X @ truth + rs.standard_normal(NOBS)]
        self.X = [[float(v) for v in X[:, j]] for j in range(n)]  # columns

    def inputs(self):
        return {f"x{j + 1}": self.X[j] for j in range(self.n)}


S3 = Data(3, 101, [0.35, -0.3, 0.25], {0, 2})
S6 = Data(6, 102, [0.35, -0.3, 0.25], {0, 3, 4})
S32 = Data(32, 103, [0.3, -0.25, 0.2, -0.35], {1, 5, 8, 13, 21, 31})
S1 = Data(1, 104, [0.4], {0})
MIX = Data(3, 105, [1.0], {0, 1})
# EDGE: S3 with its second column scaled by EDGE_SCALE.  y does not hold that column, so gamma_2's log-density
# difference lies below -800 (exp overflows, p = 0), and with gamma_2 = 1 the cross terms push another element's
# difference above 40 (p rounds to 1): both take the 0.5 branch (tests/test_binary.py checks the differences)
EDGE_SCALE = -100.0
EDGE = Data(3, 101, [0.35, -0.3, 0.25], {0, 2}, scale=[1.0, EDGE_SCALE, 1.0])

# The replay cases of tests/test_gpu_binary.py, which tests/test_binary.py runs forward alone on the same seed and
# chain counts: (data, sampler, k, chains, iterations).  8 chains x 200 iterations, and 3 chains for some: a wave's
# second half then idles on the last wave, and the paired chains take different accept branches.
LISTS = [[1], [2, 3], [4, 5, 6]]
REPLAY_CASES = [("S6", "bmc3", 1, 8, 200), ("S6", "bmc3", 3, 3, 200), ("S6", "bmc3", 6, 8, 200),
                ("S6", "bmc3", LISTS, 3, 200), ("S32", "bmc3", 5, 8, 200),
                ("S6", "bmg", 1, 3, 200), ("S6", "bmg", 3, 8, 200), ("S6", "bmg", 6, 3, 200),
                ("S6", "bmg", LISTS, 8, 200), ("S32", "bmg", 5, 3, 200), ("S1", "bmg", 1, 8, 200)]
BIA_CASES = [("S6", "bia", 1, 8, 40), ("S32", "bia", 1, 8, 40)]
EDGE_CASE = ("EDGE", "bmg", 3, 8, 200)


def prior_of(dname):
    return "uniform" if dname == "S32" else "bernoulli"


def _node_fn(ir, D, sampled_coef, prior):
    """The closure of y with the sum written out with gamma[j] elements; its signature names the nodes it reads."""
    names = ["gamma"] + [f"x{j + 1}" for j in range(D.n)] + (["beta", "s2"] if sampled_coef else [])

    def f(*a):
        g, xs = a[0], a[1:1 + D.n]
        coef = (lambda j: a[1 + D.n][j + 1]) if sampled_coef else (lambda j: D.b0[j])
        mu = xs[0] * coef(0) * g[1]
        for j in range(1, D.n):
            mu = mu + xs[j] * coef(j) * g[j + 1]
        return ir.Normal(mu, ir.sqrt(a[2 + D.n]) if sampled_coef else 1.0)
    f.__signature__ = inspect.Signature([inspect.Parameter(nm, inspect.Parameter.POSITIONAL_OR_KEYWORD) for nm in names])
    return f


def model(ir, D, prior="bernoulli", mixed=False):
    """(model, inputs, inits(K)); every sampled node is monitored.  Inits: chain k starts at the bits of a
    multiplicative hash of k, so the chains cover the states."""
    gam = ir.Stochastic(1, (lambda: ir.Bernoulli(0.5)) if prior == "bernoulli" else (lambda: ir.DiscreteUniform(0, 1)))
    nodes = dict(y=ir.Stochastic(1, _node_fn(ir, D, mixed, prior), False), gamma=gam)
    if mixed:
        nodes["beta"] = ir.Stochastic(1, lambda: ir.Normal(0.0, 10.0))
        nodes["s2"] = ir.Stochastic(lambda: ir.InverseGamma(2.0, 2.0))
    m = ir.Model(**nodes)

    def inits(K):
        out = []
        for k in range(K):
            h = (k * 2654435761 + 12345) & 0xffffffff
            d = {"y": D.y, "gamma": [float((h >> (j % 32)) & 1) if D.n > 3 else float((k >> j) & 1) for j in range(D.n)]}
            if mixed:
                d["beta"] = [1.0 + 0.05 * k, 0.9 - 0.03 * k, 0.1 * (k % 3)]
                d["s2"] = 1.0 + 0.1 * k
            out.append(d)
        return out
    return m, D.inputs(), inits


def logf_of(D, mixed=False):
    """st -> logpdf!(block of gamma): the prior terms of gamma, then the terms of its one target y."""
    def logf(st):
        g = st["gamma"]
        coef = st["beta"] if mixed else D.b0
        sd = math.sqrt(st["s2"][0]) if mixed else 1.0
        terms = [math.log(0.5)] * D.n
        on = [j for j in range(D.n) if g[j] != 0.0]  # (a product with gamma_j = 0 adds an exact zero)
        for i in range(NOBS):
            mu = math.fsum(D.X[j][i] * coef[j] * g[j] for j in on)
            terms.append(normal_lp(D.y[i], mu, sd))
        return math.fsum(terms)
    return logf


def spec(D, kind, k=1, mixed=False, first=True, **kw):
    node = BNode("gamma", D.n, logf_of(D, mixed), kind, k, **kw)
    if not mixed:
        return Spec([("bin", node)], {"gamma": (0, D.n)})
    # monitored columns follow the declaration order: gamma, beta, s2; the scheme's other blocks are RWM(beta), Slice(s2)
    cols = {"gamma": (0, D.n), "beta": (D.n, 3), "s2": (D.n + 3, 1)}
    others = [("other", ["beta"]), ("other", ["s2"])]
    return Spec([("bin", node)] + others if first else others + [("bin", node)], cols)


def logpdf_gamma_y(D, g):
    """logpdf of nodes gamma and y at gamma: (sum, sum of absolute terms)."""
    terms = [math.log(0.5)] * D.n
    for i in range(NOBS):
        terms.append(normal_lp(D.y[i], math.fsum(D.X[j][i] * D.b0[j] * g[j] for j in range(D.n)), 1.0))
    return math.fsum(terms), math.fsum(abs(t) for t in terms)
