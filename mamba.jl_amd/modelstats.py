"""Model-based posterior statistics of the device-kept draws (src/output/modelstats.jl).

logpdf(mc, nodekeys) (modelstats.jl:30-68) relists every kept draw into the model and sums the
log densities of the listed Stochastic nodes; dic(mc) (modelstats.jl:3-12) combines the mean and
the variance of the deviance D = -2 logpdf over all draws with the deviance at the posterior
means (modelstats.jl:15-25).  The evaluation runs on the GPU (modelstats.hip: mmb_draws_logpdf,
mmb_draws_deviance, mmb_logpdf_at) on the draws the engine kept; this module decides which nodes
are needed, maps names to the engine's node ids and applies the closing formulas.

Which sampled nodes a node list needs (getsimkeys, modelstats.jl:107-132): every sampled node
that a listed node's distribution parameters read, through Logical nodes, and every listed node
that is itself sampled.  They must be monitored, or the draws cannot be relisted (the reference's
names2inds fails too).  One equivalence: the reference relists a *monitored* Logical from the
chain; here a Logical is recomputed from its parents through the inlined expression -- the same
function of the draw, but its parents must be monitored.

predict(mc, nodekeys) (modelstats.jl:71-102) draws rand(node) of the observed output nodes at every
kept draw.  The reference draws from Julia's global RNG; here a predicted value is a pure function
of (seed, global chain id, iteration of the kept row, node id, element) on Philox streams of its own
(predict.hip, include/mamba_hip.h), so it does not depend on sharding, chunking or call order.
"""
import re

import numpy as np

from .samplers import ArgumentError

DIC_ROWS = ["pD", "pV"]
DIC_COLS = ["DIC", "Effective Parameters"]
PREDICT_COLS = ["Mean", "SD"]


def _keys(model, nodekeys, default):
    if nodekeys is None:
        nodekeys = model.keys(default)
    if isinstance(nodekeys, str):
        nodekeys = [nodekeys]
    nodekeys = list(nodekeys)
    if not nodekeys:
        raise ArgumentError("no nodes to evaluate")
    return nodekeys


def needed_nodes(model, nodekeys):
    """The sampled nodes whose draws the log densities of `nodekeys` need, in the model's node
    order: the listed nodes that are sampled and the sampled parents of every listed node."""
    t = model.stats_table()
    nodekeys = _keys(model, nodekeys, "stochastic")
    need = set()
    for key in nodekeys:
        if key not in t["ids"]:
            raise ArgumentError(f"{key} is not a Stochastic node of this model: " + ", ".join(t["stoch"]))
        if key in t["sampled"]:
            need.add(key)
        need |= set(t["parents"][key])
    return [n for n in t["stoch"] if n in need]


def node_ids(model, nodekeys):
    """Engine node ids of `nodekeys`, after checking that every node they need is monitored."""
    t = model.stats_table()
    nodekeys = _keys(model, nodekeys, "stochastic")
    for n in needed_nodes(model, nodekeys):
        if n not in t["monitored"]:
            raise ArgumentError(f"node {n} is not monitored: the log densities of {', '.join(nodekeys)} need its "
                                "draws in the chains")
    return np.array([t["ids"][k] for k in nodekeys], dtype=np.int32)


def _engine_call(model, f, *args):
    """Run an engine entry point; its "not monitored" refusal becomes an ArgumentError naming the node."""
    try:
        return f(*args)
    except RuntimeError as err:
        m = re.search(r"node id (\d+) is not monitored", str(err))
        if m is None:
            raise
        ids = model.stats_table()["ids"]
        name = next((k for k, v in ids.items() if v == int(m.group(1))), m.group(1))
        raise ArgumentError(f"node {name} is not monitored: the requested log densities need its draws "
                            "in the chains") from None


def logpdf_sharded(engine, model, nodekeys=None):
    """logpdf(mc, nodekeys) of this engine's kept draws: n x 1 x K (modelstats.jl:30-68)."""
    ids = node_ids(model, nodekeys)
    lp = _engine_call(model, engine.draws_logpdf, ids)
    return lp.reshape(lp.shape[0], 1, lp.shape[1], order="F")


def logpdf(sim, nodekeys=None):
    """logpdf(mc[, nodekeys]) (modelstats.jl:28-51): a Chains n x 1 x K named ["logpdf"] with
    `sim`'s start, thin and chains; nodekeys defaults to every Stochastic node, and may be one name."""
    from .mcmc import Chains
    if sim.model is None:
        raise ArgumentError("logpdf needs the model of the chains")
    node_ids(sim.model, nodekeys)  # argument errors come before the engine is asked for
    value = logpdf_sharded(sim._device_engine(), sim.model, nodekeys)
    return Chains(value, ["logpdf"], sim.start, sim.thin, sim.chains, sim.model, None)


def dic_sharded(engine, model, allreduce_sum=None):
    """dic(mc) (modelstats.jl:3-12) over every chain of every rank, from device-kept draws:
    (value 2 x 2 = [Dhat + 2p, p] with p = [mean(D) - Dhat, 0.5 var(D)], DIC_ROWS, DIC_COLS).

    Pooled means of the monitored columns (two shifted passes of mmb_chain_summary, sums
    all-reduced), Dhat = -2 logpdf at the means, then the per-chain sums of D - Dhat and its
    square (mmb_draws_deviance), one all-reduce of [S1, S2, N].  Dhat is the same on every rank,
    so the partials are additive: pD = S1 / N, var(D) = (S2 - S1^2 / N) / (N - 1)."""
    red = (lambda v: np.asarray(allreduce_sum(np.asarray(v, dtype=np.float64)), dtype=np.float64)) \
        if allreduce_sum is not None else (lambda v: np.asarray(v, dtype=np.float64))
    if getattr(model, "discrete", None):
        # Dhat is the deviance at the posterior means (modelstats.jl:15-25), and the mean of a sampled
        # discrete node is no point of its support: the reference's x[T] throws on a fractional index
        raise ArgumentError("dic: the posterior mean of a sampled discrete node (" + ", ".join(model.discrete) +
                            ") is outside its support, so the deviance at the means is undefined")
    ids = node_ids(model, model.keys("output"))
    n, K, p = engine.num_kept(), engine.K, engine.pmon
    if n < 1:
        raise ArgumentError("dic runs on the device-kept draws: sample with keep_device=True")
    from .summary import F_S1
    N = float(red([float(n) * K])[0])
    mu = np.zeros(p)
    for _ in range(2):  # shifted by 0, then by the first mean: the sum of the residuals refines it
        s1 = red(engine.chain_summary(mu, n, 0)[:, :, F_S1].sum(0))
        mu = mu + s1 / N
    dhat = -2.0 * float(_engine_call(model, engine.logpdf_at, ids, mu))
    acc = np.asarray(_engine_call(model, engine.draws_deviance, ids, dhat), dtype=np.float64)
    tot = red([acc[:, 0].sum(), acc[:, 1].sum(), float(n) * K])
    S1, S2, N = float(tot[0]), float(tot[1]), float(tot[2])
    pD = S1 / N
    pV = 0.5 * (S2 - S1 * S1 / N) / (N - 1.0)
    pvec = np.array([pD, pV])
    return np.column_stack([dhat + 2.0 * pvec, pvec]), list(DIC_ROWS), list(DIC_COLS)


def dic(sim):
    """dic(mc) (modelstats.jl:3-12): (value 2 x 2, ["pD", "pV"], ["DIC", "Effective Parameters"])."""
    if sim.model is None:
        raise ArgumentError("dic needs the model of the chains")
    return dic_sharded(sim._device_engine(), sim.model)


# ---------------------------------------------------------------- predict (modelstats.jl:71-102)
def predict_keys(model, nodekeys=None):
    """The node list of a predict call: `nodekeys` (default keys(m, :output), may be one name), every
    one an output node, or the reference's ArgumentError (modelstats.jl:78-82, its message verbatim,
    the typo "nodess" included)."""
    nodekeys = _keys(model, nodekeys, "output")
    outputs = model.keys("output")
    if not all(k in outputs for k in nodekeys):
        raise ArgumentError("nodekeys are not all observed Stochastic nodess : " + ", ".join(outputs))
    for k in nodekeys:  # node-IR models: variates the predict kernel does not draw
        why = getattr(model, "no_predict", {}).get(k)
        if why:
            raise ArgumentError(f"predict: node {k} is {why}: its variates are not lowered")
    return nodekeys


def predict_names(model, nodekeys):
    """names(m, nodekeys): y[1], y[2], ... per element, a scalar node by its bare name."""
    t = model.stats_table()
    return [nm for k in nodekeys for nm in t["names"][k]]


def _observed(model, nodekeys):
    """The listed nodes' observed values, in result-column order."""
    obs = model.stats_table().get("observed", {})
    parts = []
    for k in nodekeys:
        v = obs[k] if k in obs else (model.inputs or {}).get(k)
        if v is None:
            raise ArgumentError(f"no observed values for node {k}: set the model's inputs")
        parts.append(np.asarray(v, dtype=np.float64).ravel())
    return np.concatenate(parts)


def _predict_seed(engine, seed):
    return int(engine.seed if seed is None else seed)


def predict_sharded(engine, model, nodekeys=None, seed=None, start=1, thin=1, rows=None):
    """predict(mc, nodekeys) of this engine's kept draws: (value n x P x K, names).  Kept row i has
    iteration start + i * thin; `rows` = (i0, i1) gives the kept rows [i0, i1) only.  Global chain
    ids key the streams, so the shards of a run predict what one engine over all chains predicts."""
    keys = predict_keys(model, nodekeys)
    ids = node_ids(model, keys)
    i0, i1 = (0, engine.num_kept()) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= i0 < i1 <= engine.num_kept():
        raise ArgumentError(f"rows [{i0}, {i1}) are not inside the {engine.num_kept()} kept draws")
    value = _engine_call(model, engine.draws_predict, ids, _predict_seed(engine, seed), int(start), int(thin), i0, i1)
    return value, predict_names(model, keys)


def predict(sim, nodekeys=None, seed=None, rows=None):
    """predict(mc[, nodekeys]) (modelstats.jl:71-102): a Chains n x P x K of posterior predictive
    draws, named names(m, nodekeys), with `sim`'s start (shifted to the first of `rows`), thin,
    chains and model.  `seed` defaults to the seed the chains were initialised with."""
    from .mcmc import Chains
    if sim.model is None:
        raise ArgumentError("predict needs the model of the chains")
    keys = predict_keys(sim.model, nodekeys)
    node_ids(sim.model, keys)  # argument errors come before the engine is asked for
    value, names = predict_sharded(sim._device_engine(), sim.model, keys, seed, sim.start, sim.thin, rows)
    i0 = 0 if rows is None else int(rows[0])
    return Chains(value, names, sim.start + i0 * sim.thin, sim.thin, sim.chains, sim.model, None)


def predict_moments_sharded(engine, model, nodekeys=None, allreduce_sum=None, seed=None, start=1, thin=1):
    """Pooled P x [Mean, SD] of the predicted values over every chain of every rank; they never leave
    the device.  The per-chain sums of (yhat - y) and its square about the node's observed data y (a
    shift every rank shares, near the values, so nothing cancels) come from mmb_draws_predict_moments;
    one all-reduce of [S1, S2, N]: Mean = y + S1 / N, SD = sqrt((S2 - S1^2 / N) / (N - 1))."""
    red = (lambda v: np.asarray(allreduce_sum(np.asarray(v, dtype=np.float64)), dtype=np.float64)) \
        if allreduce_sum is not None else (lambda v: np.asarray(v, dtype=np.float64))
    keys = predict_keys(model, nodekeys)
    ids = node_ids(model, keys)
    n, K = engine.num_kept(), engine.K
    if n < 1:
        raise ArgumentError("predict runs on the device-kept draws: sample with keep_device=True")
    shift = _observed(model, keys)
    acc = np.asarray(_engine_call(model, engine.draws_predict_moments, ids, _predict_seed(engine, seed), int(start),
                                  int(thin), shift), dtype=np.float64)
    P = acc.shape[1]
    tot = red(np.concatenate([acc[:, :, 0].sum(0), acc[:, :, 1].sum(0), [float(n) * K]]))
    S1, S2, N = tot[:P], tot[P:2 * P], float(tot[2 * P])
    var = (S2 - S1 * S1 / N) / (N - 1.0) if N > 1.0 else np.full(P, np.nan)
    return np.column_stack([shift + S1 / N, np.sqrt(var)])


def predict_summary(sim, nodekeys=None, seed=None):
    """(P x 2 [Mean, SD] of predict(mc, nodekeys) pooled over draws and chains, names, ["Mean", "SD"])."""
    if sim.model is None:
        raise ArgumentError("predict needs the model of the chains")
    keys = predict_keys(sim.model, nodekeys)
    value = predict_moments_sharded(sim._device_engine(), sim.model, keys, None, seed, sim.start, sim.thin)
    return value, predict_names(sim.model, keys), list(PREDICT_COLS)
