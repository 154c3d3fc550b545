"""DGS (src/samplers/dgs.jl:109-126) restated in plain Python: the checker of tests/test_gpu_dgs.py.

    for element i of the node, in order:
        mass_k = exp(logpdf(d_i, s_k) + logpdf(model, node.targets))  for the k-th support value s_k
        psum   = mass_0 + mass_1 + ...
        probs  = psum > 0 ? mass / psum : 1 / n
        value  = the smallest k with probs_0 + ... + probs_k > u (the last one if none),
                 u = uniform #i of the block's MMB_SUB_UNIFORM stream

The log densities are the test models' own formulas written out below with math.lgamma / math.log /
math.fsum, and the masses math.exp of them: no project code except `orc_uniform` of the oracle library
for u.  It is a reference, not a second copy of the device's summation order, so the comparison is
decision-exact away from thresholds: where u lies within DELTA of one of the restatement's cumulative
probabilities the device may choose either adjacent value; the replay then adopts the device's choice
and counts a skip.  (In the test models the absolute log-density terms sum to at most 1e4; a rounded
sum of a few hundred terms is within about 1e2 * 2^-53 * 1e4 ~ 1e-10 of exact, two orders under DELTA.)
A psum that is not finite has no probability vector (the reference throws): the element keeps its value.

A model description (`Spec`) lists, per discrete node: its length, support(i) -> the ascending values,
own(i, v, st) -> logpdf(d_i, v), and targets(st) -> the element terms of logpdf(model, node.targets);
`st` maps node names to lists of floats.  The second half of this file holds the test models: the
node-IR definition (built on the `ir` module the caller passes) next to its formulas.
"""
import math

SUB_UNIFORM = 1
DELTA = 1e-8
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def normal_lp(x, mu, sigma):
    z = (x - mu) / sigma
    return -0.5 * z * z - HALF_LOG_2PI - math.log(sigma)


def poisson_lp(k, lam):
    return (k * math.log(lam) if k else 0.0) - lam - math.lgamma(k + 1.0)


def binomial_lp(k, n, p):
    return (math.lgamma(n + 1.0) - math.lgamma(k + 1.0) - math.lgamma(n - k + 1.0) +
            (k * math.log(p) if k else 0.0) + ((n - k) * math.log1p(-p) if n - k else 0.0))


def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


class DNode:
    def __init__(self, name, length, support, own, targets):
        self.name, self.length, self.support, self.own, self.targets = name, length, support, own, targets


class Spec:
    """blocks: the scheme in device block order, each ("dgs", DNode) or ("other", [node names])."""

    def __init__(self, blocks, columns):
        self.blocks = blocks
        self.columns = columns  # node name -> (first monitored column, length)


def conditional(node, i, st):
    """(support, probs or None) of element i given the state: dgs.jl:109-126 mass and its normalisation."""
    sup = node.support(i)
    old = st[node.name][i]
    mass = []
    for v in sup:
        st[node.name][i] = float(v)
        terms = [node.own(i, v, st)] + list(node.targets(st))
        lp = -math.inf if any(t == -math.inf for t in terms) else math.fsum(terms)
        mass.append(_exp(lp))
    st[node.name][i] = old
    psum = 0.0
    for m in mass:
        psum = psum + m
    if not math.isfinite(psum):
        return sup, None
    n = len(sup)
    return sup, [m / psum if psum > 0.0 else 1.0 / n for m in mass]


def choose(probs, u):
    """(index chosen, near): near = the index pair (k, k + 1) of a cumulative probability within DELTA
    of u, else None."""
    cum, pick, near = 0.0, len(probs) - 1, None
    found = False
    for k, p in enumerate(probs):
        cum = cum + p
        if k < len(probs) - 1 and abs(cum - u) <= DELTA:
            near = (k, k + 1)
        if not found and cum > u:
            pick, found = k, True
    return pick, near


class Replay:
    """Replays chains from their inits update by update against the device's draws (thin 1, burnin 0,
    every node monitored): draws[t, column, chain]."""

    def __init__(self, orc_uniform, spec, seed, chain_offset=0):
        self.u, self.spec, self.seed, self.off = orc_uniform, spec, seed, chain_offset
        self.skips = 0
        self.updates = 0
        self.mismatch = []

    def state(self, row):
        return {n: [float(x) for x in row[c0:c0 + ln]] for n, (c0, ln) in self.spec.columns.items()}

    def chain(self, c, init_row, draws, it0=0):
        """init_row: the chain's initial values in monitored-column order; draws[:, :, c] its kept draws."""
        st = self.state(init_row)
        for t in range(draws.shape[0]):
            dev = self.state(draws[t, :, c])
            for b, (kind, what) in enumerate(self.spec.blocks):
                if kind != "dgs":  # another sampler's block: its new values are the draw's
                    for n in what:
                        st[n] = list(dev[n])
                    continue
                for i in range(what.length):
                    self.updates += 1
                    got = dev[what.name][i]
                    sup, probs = conditional(what, i, st)
                    if probs is None:
                        want, near = st[what.name][i], None
                    else:
                        u = self.u(self.seed, self.off + c, it0 + t + 1, b, SUB_UNIFORM, i)
                        k, near = choose(probs, u)
                        want = float(sup[k])
                    if got != want:
                        if near is not None and got in (float(sup[near[0]]), float(sup[near[1]])):
                            self.skips += 1
                        else:
                            self.mismatch.append((c, it0 + t + 1, what.name, i, got, want))
                    st[what.name][i] = got  # continue from the device's state
        return st

    def run(self, init, draws, it0=0):
        for c in range(draws.shape[2]):
            self.chain(c, init[c], draws, it0)
        return self


def forward(orc_uniform, spec, seed, init_row, chain, iters):
    """The restatement alone (pure-DGS schemes): (draw rows, thresholds met): the number of updates
    whose u lies within DELTA of a cumulative probability."""
    R = Replay(orc_uniform, spec, seed)
    st = R.state(init_row)
    near_hits, rows = 0, []
    for t in range(iters):
        for b, (kind, node) in enumerate(spec.blocks):
            assert kind == "dgs"
            for i in range(node.length):
                sup, probs = conditional(node, i, st)
                if probs is None:
                    continue
                k, near = choose(probs, orc_uniform(seed, chain, t + 1, b, SUB_UNIFORM, i))
                near_hits += near is not None
                st[node.name][i] = float(sup[k])
        row = [0.0] * sum(ln for _, ln in spec.columns.values())
        for n, (c0, ln) in spec.columns.items():
            row[c0:c0 + ln] = st[n]
        rows.append(row)
    return rows, near_hits


# ------------------------------------------------------------------ the test models
# Each returns (model, inputs, inits(K), scheme(mb), spec(scheme order)); every sampled node is monitored.

M1_G = [1.0, 1, 2, 2, 3, 3]
M1_Y = [0.3, 1.9, -0.4, 0.2, 2.6, 1.1]
M1_M0, M1_D = 0.25, 1.5


def model1(ir):
    """z ~ Bernoulli(0.3) (3), y_j ~ Normal(m0 + d z[g_j], 1) (6): a data-index gather (VALG)."""
    m = ir.Model(
        y=ir.Stochastic(1, lambda z, g, m0, d: ir.Normal(m0 + d * z[g], 1.0), False),
        z=ir.Stochastic(1, lambda: ir.Bernoulli(0.3)))
    inputs = {"g": M1_G, "m0": M1_M0, "d": M1_D}

    def inits(K):
        return [{"y": M1_Y, "z": [(k >> j) & 1 for j in range(3)]} for k in range(K)]
    return m, inputs, inits


def model1_lp(z):
    """log joint of model 1 at z (3 values in {0, 1})."""
    terms = [math.log(0.3) if v == 1 else math.log(1.0 - 0.3) for v in z]
    terms += [normal_lp(M1_Y[j], M1_M0 + M1_D * z[int(M1_G[j]) - 1], 1.0) for j in range(6)]
    return math.fsum(terms)


def spec1():
    z = DNode("z", 3, lambda i: [0, 1],
              lambda i, v, st: math.log(0.3) if v == 1 else math.log(1.0 - 0.3),
              lambda st: [normal_lp(M1_Y[j], M1_M0 + M1_D * st["z"][int(M1_G[j]) - 1], 1.0) for j in range(6)])
    return Spec([("dgs", z)], {"z": (0, 3)})


M2_P = [0.4, 0.35, 0.25]
M2_MU = [-1.0, 0.5, 2.0]
M2_S = 0.8
M2_N = 40
M2_Y = [M2_MU[(7 * j + j // 3) % 3] + 0.9 * math.sin(1.7 * j + 0.3) for j in range(M2_N)]


def model2(ir):
    """T ~ Categorical(p) (40 elements: more than a lane group), y ~ Normal(mu[T], s), mu data (DATAV)."""
    m = ir.Model(
        y=ir.Stochastic(1, lambda mu, T, s: ir.Normal(mu[T], s), False),
        T=ir.Stochastic(1, lambda: ir.Categorical(M2_P)))
    inputs = {"mu": M2_MU, "s": M2_S}

    def inits(K):
        return [{"y": M2_Y, "T": [(k + j) % 3 + 1 for j in range(M2_N)]} for k in range(K)]
    return m, inputs, inits


def _t_node(mu_of):
    return DNode("T", M2_N, lambda i: [1, 2, 3],
                 lambda i, v, st: math.log(M2_P[int(v) - 1]),
                 lambda st: [normal_lp(M2_Y[j], mu_of(st)[int(st["T"][j]) - 1], M2_S) for j in range(M2_N)])


def spec2():
    return Spec([("dgs", _t_node(lambda st: M2_MU))], {"T": (0, M2_N)})


def model2_logpdf(T):
    """logpdf of nodes T and y of model 2 at T: (sum, sum of absolute terms)."""
    terms = [math.log(M2_P[int(v) - 1]) for v in T] + \
            [normal_lp(M2_Y[j], M2_MU[int(T[j]) - 1], M2_S) for j in range(M2_N)]
    return math.fsum(terms), math.fsum(abs(t) for t in terms)


def model3(ir):
    """Model 2 with mu a sampled 3-vector, mu ~ Normal(0, 10): mu[T] gathers from the state (VALV)."""
    m = ir.Model(
        y=ir.Stochastic(1, lambda mu, T, s: ir.Normal(mu[T], s), False),
        T=ir.Stochastic(1, lambda: ir.Categorical(M2_P)),
        mu=ir.Stochastic(1, lambda: ir.Normal(0.0, 10.0)))
    inputs = {"s": M2_S}

    def inits(K):
        return [{"y": M2_Y, "T": [(k + j) % 3 + 1 for j in range(M2_N)],
                 "mu": [M2_MU[0] + 0.1 * k, M2_MU[1] - 0.05 * k, M2_MU[2] + 0.02 * k]} for k in range(K)]
    return m, inputs, inits


def spec3(dgs_first):
    t = ("dgs", _t_node(lambda st: st["mu"]))
    o = ("other", ["mu"])
    return Spec([t, o] if dgs_first else [o, t], {"T": (0, M2_N), "mu": (M2_N, 3)})


M4_N = [3.0, 5.0]
M4_R = [4.0, 9.0]
M4_M = [0.0, 0.4, 0.9, 1.3, 2.2, 2.4, 3.1, 3.3, 4.0, 4.8]
M4_Y = [1.1, 2.5, 3.2]


def model4(ir):
    """k ~ Binomial(n, 0.4), n = [3, 5] (per-element supports), r ~ Poisson(1 + 2 k) observed;
    tau ~ DiscreteUniform(1, 10) (3), y ~ Normal(m[tau], 1)."""
    m = ir.Model(
        r=ir.Stochastic(1, lambda k: ir.Poisson(1.0 + 2.0 * k), False),
        k=ir.Stochastic(1, lambda n: ir.Binomial(n, 0.4)),
        y=ir.Stochastic(1, lambda m, tau: ir.Normal(m[tau], 1.0), False),
        tau=ir.Stochastic(1, lambda: ir.DiscreteUniform(1, 10)))
    inputs = {"n": M4_N, "m": M4_M}

    def inits(K):
        return [{"r": M4_R, "y": M4_Y, "k": [k % 4, k % 6], "tau": [1 + k % 10, 1 + (3 * k) % 10, 10 - k % 10]}
                for k in range(K)]
    return m, inputs, inits


def spec4():
    k = DNode("k", 2, lambda i: list(range(int(M4_N[i]) + 1)),
              lambda i, v, st: binomial_lp(v, M4_N[i], 0.4),
              lambda st: [poisson_lp(M4_R[j], 1.0 + 2.0 * st["k"][j]) for j in range(2)])
    tau = DNode("tau", 3, lambda i: list(range(1, 11)),
                lambda i, v, st: -math.log(10.0),
                lambda st: [normal_lp(M4_Y[j], M4_M[int(st["tau"][j]) - 1], 1.0) for j in range(3)])
    return Spec([("dgs", k), ("dgs", tau)], {"k": (0, 2), "tau": (2, 3)})


def model5(ir):
    """z ~ Bernoulli(0.5) whose only target is y = 100 ~ Normal(z, 1e-3): every mass underflows to 0."""
    m = ir.Model(
        y=ir.Stochastic(lambda z: ir.Normal(z, 1e-3), False),
        z=ir.Stochastic(lambda: ir.Bernoulli(0.5)))

    def inits(K):
        return [{"y": 100.0, "z": k % 2} for k in range(K)]
    return m, {}, inits


def spec5():
    z = DNode("z", 1, lambda i: [0, 1], lambda i, v, st: math.log(0.5),
              lambda st: [normal_lp(100.0, st["z"][0], 1e-3)])
    return Spec([("dgs", z)], {"z": (0, 1)})
