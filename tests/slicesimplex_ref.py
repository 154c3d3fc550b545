"""SliceSimplex (src/samplers/slicesimplex.jl:86-122) restated on the oracle's primitives: the checker of
tests/test_gpu_slicesimplex.py.

One update of a Dirichlet node of k elements at value v (block b of iteration `it`, chain c; indices from 0,
every sum in index order from 0.0):

    draw r        w_j = e_j / (e_0 + ... + e_{k-1}), e_j = -log(1 - u), u = uniform #(32 r + j) of the block's
                  SUB_SIMPLEX stream
    p0            logf(v) + log(uniform #0 of SUB_UNIFORM)
    first simplex V0[i][j] = I[i][j] + (1 - scale) (I[i][0] - I[i][j]);  V[i][j] = (V0[i][j] + v_i) - (V0 w)_i
                  with w = draw 0;  bx = w  (= V \\ v exactly)
    candidate r   xb = draw r, x = V xb; rejected iff some x_i < 0, some x_i > 1, or logf(x) < p0 (logf is
                  evaluated for an in-box x only; a NaN accepts)
    shrink        bc = xb, I = {i : bc_i < bx_i} fixed first; for i in I ascending, t = bc_i (current):
                  V[:, j] += t (V[:, i] - V[:, j]) for j != i;  b_j <- b_j / (1 - t) (j != i),
                  b_i <- (b_i - t) / (1 - t) for b in (bc, bx)

The uniforms and every log of the draws are the oracle library's (`orc_uniform`, `orc_log`: the device's
Philox streams and its log, bit for bit); the vector arithmetic is numpy's elementwise IEEE double
arithmetic in the device's operation order (the device code is compiled with contraction off), so the
candidates x and the accepted draws are bit-equal to the device's.  logf(x) = logpdf(d, x) +
logpdf(model, node.targets) is the test models' own formulas (math.log / math.lgamma / math.fsum): a
reference, not the device's summation order, so the one decision that may differ is logf(x) < p0.  An
update is a *threshold skip* when some candidate has |logf(x) - p0| <= DELTA_REL x (the sum of the absolute
terms of logf(x)); the replay then continues from the device's value.

A model description (`Spec`) lists the scheme's blocks in device order, each ("ssx", SNode) or
("other", [node names]); SNode: the node's name, alpha, scale and targets(st) -> the element terms of
logpdf(model, node.targets), `st` mapping node names to lists of floats.
"""
import math

import numpy as np

SUB_UNIFORM, SUB_SIMPLEX = 1, 6
DELTA_REL = 1e-9
SIMPLEX_TOL = 1e-8
MAX_SHRINK = 100000


def _log(x):
    if x > 0.0:
        return math.log(x)
    return -math.inf if x == 0.0 else math.nan


class Prim:
    """The oracle library's primitives."""

    def __init__(self, L):
        self.u, self.log = L.orc_uniform, L.orc_log


class SNode:
    def __init__(self, name, alpha, scale, targets):
        self.name, self.alpha, self.scale, self.targets = name, [float(a) for a in alpha], float(scale), targets
        self.lmnb = math.fsum(math.lgamma(a) for a in self.alpha) - math.lgamma(math.fsum(self.alpha))


class Spec:
    def __init__(self, blocks, columns):
        self.blocks = blocks
        self.columns = columns  # node name -> (first monitored column, length)


def dirichlet_terms(alpha, lmnb, x):
    """The terms of logpdf(Dirichlet(alpha), x), or [-inf] off the support (every x_i >= 0 and
    |sum x - 1| <= SIMPLEX_TOL; a NaN fails)."""
    if not all(v >= 0.0 for v in x) or not abs(math.fsum(x) - 1.0) <= SIMPLEX_TOL:
        return [-math.inf]
    return [0.0 if a == 1.0 else (a - 1.0) * _log(v) for a, v in zip(alpha, x)] + [-lmnb]


def logf(node, st, x):
    """(logf(x), sum of the absolute terms): the node at x, then its targets with x in the state."""
    st[node.name] = [float(v) for v in x]
    own = dirichlet_terms(node.alpha, node.lmnb, st[node.name])
    tg = list(node.targets(st))
    terms = own + tg
    if any(t != t for t in terms):
        return math.nan, math.inf
    if any(t == -math.inf for t in terms):
        return -math.inf, math.inf
    return math.fsum(terms), math.fsum(abs(t) for t in terms)


def draw(prim, key, r, k):
    seed, chain, it, b = key
    e = [-prim.log(1.0 - prim.u(seed, chain, it, b, SUB_SIMPLEX, 32 * r + j)) for j in range(k)]
    s = 0.0
    for v in e:
        s = s + v
    return np.array([v / s for v in e])


def matvec(V, xb):
    acc = np.zeros(V.shape[0])
    for j in range(V.shape[1]):
        acc = acc + V[:, j] * xb[j]
    return acc


def first_simplex(v, w, scale):
    k = len(v)
    eye = np.eye(k)
    V0 = eye + (1.0 - scale) * (eye[:, [0]] - eye)
    return (V0 + np.asarray(v, dtype=np.float64)[:, None]) - matvec(V0, w)[:, None]


def shrink(V, bx, xb):
    """One shrink after the rejected candidate with coordinates xb: (V, bx) in place of the reference's
    shrinksimplex and its `vertices \\ v`."""
    k = len(bx)
    idx = [i for i in range(k) if xb[i] < bx[i]]
    bc = xb.copy()
    with np.errstate(all="ignore"):
        for i in idx:
            t = bc[i]
            om = 1.0 - t
            col = V[:, i].copy()
            V = V + t * (col[:, None] - V)
            V[:, i] = col
            ti, xi = bc[i] - t, bx[i] - t
            bc, bx = bc / om, bx / om
            bc[i], bx[i] = ti / om, xi / om
    return V, bx


def update(prim, node, st, key, solve=None):
    """One update of `node` in state `st` (st[node.name] is overwritten with the result).  Returns
    {"value", "near", "cands", "capped"}: `near` = some candidate's logf lay within the threshold band.
    `solve`, when a list, receives after the first simplex and after every shrink the largest
    |bx - numpy.linalg.solve(V, v)|."""
    v = [float(a) for a in st[node.name]]
    k = len(v)
    l0, _ = logf(node, st, v)
    p0 = l0 + prim.log(prim.u(key[0], key[1], key[2], key[3], SUB_UNIFORM, 0))
    bx = draw(prim, key, 0, k)
    V = first_simplex(v, bx, node.scale)
    out = {"value": v, "near": False, "cands": 0, "capped": False}

    def check():
        if solve is not None:
            solve.append(float(np.abs(np.linalg.solve(V, np.array(v)) - bx).max()))
    check()
    for r in range(1, MAX_SHRINK + 1):
        out["cands"] = r
        xb = draw(prim, key, r, k)
        x = matvec(V, xb)
        rej = bool(np.any(x < 0.0) or np.any(x > 1.0))
        if not rej:
            lx, mag = logf(node, st, x)
            if math.isfinite(lx) and math.isfinite(p0) and abs(lx - p0) <= DELTA_REL * mag:
                out["near"] = True
            rej = lx < p0
        if not rej:
            out["value"] = [float(a) for a in x]
            st[node.name] = list(out["value"])
            return out
        V, bx = shrink(V, bx, xb)
        check()
    out["capped"] = True
    st[node.name] = list(v)
    return out


class Replay:
    """Replays chains update by update against the device's draws (thin 1, burnin 0, every sampled node
    monitored): draws[t, column, chain].  Every SliceSimplex update starts from the device's state, so a
    mismatch does not spread."""

    def __init__(self, prim, spec, seed, chain_offset=0):
        self.prim, self.spec, self.seed, self.off = prim, spec, seed, chain_offset
        self.skips = self.updates = self.cands = 0
        self.mismatch = []

    def state(self, row):
        return {n: [float(x) for x in row[c0:c0 + ln]] for n, (c0, ln) in self.spec.columns.items()}

    def chain(self, c, init_row, draws, it0=0):
        st = self.state(init_row)
        for t in range(draws.shape[0]):
            dev = self.state(draws[t, :, c])
            for b, (kind, what) in enumerate(self.spec.blocks):
                if kind != "ssx":  # another sampler's block: its new values are the draw's
                    for n in what:
                        st[n] = list(dev[n])
                    continue
                self.updates += 1
                got = dev[what.name]
                res = update(self.prim, what, st, (self.seed, self.off + c, it0 + t + 1, b))
                self.cands += res["cands"]
                if res["value"] != got:
                    if res["near"]:
                        self.skips += 1
                    else:
                        self.mismatch.append((c, it0 + t + 1, what.name, got, res["value"]))
                st[what.name] = list(got)  # continue from the device's state
        return st

    def run(self, init, draws, it0=0):
        for c in range(draws.shape[2]):
            self.chain(c, init[c], draws, it0)
        return self


def forward(prim, spec, seed, init_row, chain, iters, solve=None):
    """The restatement alone: (draw rows, updates whose candidates met the threshold band, candidates
    drawn).  The nodes of other samplers' blocks keep their initial values."""
    R = Replay(prim, spec, seed)
    st = R.state(init_row)
    near = cands = 0
    rows = []
    for t in range(iters):
        for b, (kind, node) in enumerate(spec.blocks):
            if kind != "ssx":
                continue
            res = update(prim, node, st, (seed, chain, t + 1, b), solve)
            assert not res["capped"]
            near += res["near"]
            cands += res["cands"]
        row = [0.0] * sum(ln for _, ln in spec.columns.values())
        for n, (c0, ln) in spec.columns.items():
            row[c0:c0 + ln] = st[n]
        rows.append(row)
    return rows, near, cands


# ------------------------------------------------------------------ the test models
# Each model function returns (model, inputs, inits(K)); every sampled node is monitored.

MA_ALPHA = [1.0, 2.0, 0.5]
MA_T = [1.0] * 7 + [2.0] * 3 + [3.0] * 2
MA_POST = [8.0, 5.0, 2.5]  # alpha + counts


def _cat_terms(P, T):
    return [_log(P[int(t) - 1]) for t in T]


def _simplex_inits(k, K):
    """K starting points inside the simplex, chain c's weights c-dependent."""
    out = []
    for c in range(K):
        w = [1.0 + ((3 * c + 5 * j) % 7) for j in range(k)]
        s = math.fsum(w)
        out.append([x / s for x in w])
    return out


def modelA(ir):
    """P ~ Dirichlet([1, 2, 0.5]); T ~ Categorical(P) observed, 12 elements with counts (7, 3, 2)."""
    m = ir.Model(
        T=ir.Stochastic(1, lambda P: ir.Categorical(P), False),
        P=ir.Stochastic(1, lambda: ir.Dirichlet(MA_ALPHA)))

    def inits(K):
        return [{"T": MA_T, "P": p} for p in _simplex_inits(3, K)]
    return m, {}, inits


def specA(scale=1.0):
    P = SNode("P", MA_ALPHA, scale, lambda st: _cat_terms(st["P"], MA_T))
    return Spec([("ssx", P)], {"P": (0, 3)})


def modelA_logpdf(P):
    """logpdf of nodes P and T of model A: (sum, sum of absolute terms)."""
    node = specA().blocks[0][1]
    terms = dirichlet_terms(node.alpha, node.lmnb, list(P)) + _cat_terms(P, MA_T)
    return math.fsum(terms), math.fsum(abs(t) for t in terms)


MB_K = 32
MB_ALPHA = [(0.5, 1.0, 3.0)[j % 3] for j in range(MB_K)]
MB_T = [float(j % MB_K + 1) for j in range(40)]  # 40 elements (more than a lane group), every category present
MB_SCALE = 0.5


def modelB(ir):
    """k = 32 (a full lane group), alpha alternating 0.5 / 1 / 3 as a data vector, T observed."""
    m = ir.Model(
        T=ir.Stochastic(1, lambda P: ir.Categorical(P), False),
        P=ir.Stochastic(1, lambda alpha: ir.Dirichlet(alpha)))

    def inits(K):
        return [{"T": MB_T, "P": p} for p in _simplex_inits(MB_K, K)]
    return m, {"alpha": MB_ALPHA}, inits


def specB():
    P = SNode("P", MB_ALPHA, MB_SCALE, lambda st: _cat_terms(st["P"], MB_T))
    return Spec([("ssx", P)], {"P": (0, MB_K)})


MC_Y = [529.0, 530.0, 532.0, 549.4, 551.4, 552.8]
MC_SCALE = 0.75


def modelC(ir):
    """eyes (doc/examples/eyes.jl) with 6 observations, every sampled node monitored."""
    m = ir.eyes_model(monitor_all=True)

    def inits(K):
        two = ir.eyes_inits(MC_Y)
        return [two[c % 2] for c in range(K)]
    return m, ir.eyes_inputs(), inits


def specC(reverse=False):
    """Scheme order of doc/examples/eyes.jl:74-77, or reversed; columns in the model's declaration order:
    T (6), P (2), lam (2, a Logical: not state), lambda0, theta, s2."""
    P = SNode("P", [1.0, 1.0], MC_SCALE, lambda st: _cat_terms(st["P"], st["T"]))
    blocks = [("other", ["T"]), ("other", ["lambda0", "theta"]), ("other", ["s2"]), ("ssx", P)]
    n = len(MC_Y)
    cols = {"T": (0, n), "P": (n, 2), "lambda0": (n + 4, 1), "theta": (n + 5, 1), "s2": (n + 6, 1)}
    return Spec(blocks[::-1] if reverse else blocks, cols)
