"""Posterior predictive draws on the device (predict.hip through mmb_draws_predict /
mmb_draws_predict_moments, mamba.jl_amd/modelstats.py) against the restatement tests/predict_ref.py.

The fixtures and their expected values come from tests/test_predict.py (computed once per session),
which also asserts that no discrete draw of them sits on a cdf step.  So: the discrete families must
be exactly equal; the continuous ones agree to rtol 1e-12 + atol 1e-9, the project's bound in
tests/test_gpu_modelstats.py (a parameter may differ from the restatement's by ulps, the variates' z
and u are bit-identical); NaN positions are identical.  Draws are uploaded with set_draws."""
import threading

import numpy as np
import pytest

import predict_ref as ref
import test_predict as tp
from test_gpu_modelstats import ir_engine, ir_line, ir_rats, ir_seeds, line_engine
from test_modelstats import _SumOverRanks
from test_predict import LINE_START as START, LINE_THIN as THIN, SEED, fixture

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-12, 1e-9


def same(got, want, d=None, keys=None):
    """NaN positions identical; discrete columns exactly equal, the others within the bound."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    disc = np.zeros(want.shape[1], dtype=bool)
    if d is not None:
        j = 0
        for k in keys:
            nd = d["nodes"][k]
            disc[j:j + nd["len"]] = nd["fam"] in ref.DISCRETE
            j += nd["len"]
    assert np.array_equal(got[:, disc, :], want[:, disc, :], equal_nan=True)
    g, w = got[:, ~disc, :], want[:, ~disc, :]
    ok = ~np.isnan(w)
    np.testing.assert_allclose(g[ok], w[ok], rtol=RTOL, atol=ATOL)


def allfam_engine(mamba, monkeypatch, K, off=0):
    m = tp.allfam_model(mamba)
    V = m.init_matrix(tp.allfam_inits(K), K)
    monkeypatch.setenv("MMB_IR_JIT", "0")
    eng = mamba.Engine(m)
    eng.init_chains(V, chain_offset=off, seed=SEED)
    return m, eng


def ids_of(mamba, m, keys):
    return mamba.modelstats.node_ids(m, keys)


# ---------------------------------------------------------------- against the restatement
def test_line_hand_lowered(mamba):
    v, d, keys, want, _ = fixture("line")
    m, eng = line_engine(mamba, v.shape[2])
    eng.set_draws(v)
    assert eng.predict_width([mamba.abi.MMB_LINE_Y]) == 5
    got = eng.draws_predict([mamba.abi.MMB_LINE_Y], SEED, START, THIN)
    assert got.shape == (5, 5, 70)
    same(got, want)
    sim = mamba.Chains(v, m.monitor_names, START, THIN, np.arange(1, 71), m, eng)
    pp = sim.predict()                           # the chains' own seed is SEED
    assert pp.names == [f"y[{i}]" for i in range(1, 6)] and pp.range == sim.range
    assert np.array_equal(pp.value, got, equal_nan=True)


def test_ir_line(mamba, monkeypatch):
    v, d, keys, want, _ = fixture("ir_line")
    m, V = ir_line(mamba, v.shape[2])
    eng = ir_engine(mamba, monkeypatch, m, V)
    eng.set_draws(v)
    same(eng.draws_predict(ids_of(mamba, m, keys), SEED, START, THIN), want, d, keys)


def test_ir_seeds(mamba, monkeypatch):
    v, d, keys, want, _ = fixture("seeds")
    m, V = ir_seeds(mamba, v.shape[2])
    eng = ir_engine(mamba, monkeypatch, m, V)
    eng.set_draws(v)
    got = eng.draws_predict(ids_of(mamba, m, keys), SEED, START, THIN)
    assert got.shape == (5, 21, 70)
    assert np.array_equal(got, want)             # Binomial: exactly equal
    assert np.all(got <= np.asarray(mamba.ir.SEEDS["n"], float)[None, :, None])


def test_ir_rats_partial_tile(mamba, monkeypatch):
    v, d, keys, want, _ = fixture("rats")        # K = 33: a tile of 32 chains and one of 1
    m, V = ir_rats(mamba, v.shape[2])
    eng = ir_engine(mamba, monkeypatch, m, V)
    eng.set_draws(v)
    got = eng.draws_predict(ids_of(mamba, m, keys), SEED, START, THIN)
    assert got.shape == (3, 150, 33)
    same(got, want, d, keys)


def test_every_family(mamba, monkeypatch):
    v, d, keys, want, _ = fixture("allfam")
    m, eng = allfam_engine(mamba, monkeypatch, v.shape[2])
    eng.set_draws(v)
    got = eng.draws_predict(ids_of(mamba, m, keys), SEED, START, THIN)
    same(got, want, d, keys)
    # a node list in another order: the same values in other columns (streams are keyed by the node id)
    sub = ["yp", "yg", "ybi"]
    j = dict(zip(keys, np.cumsum([0] + ref.widths(d, keys))))
    pick = np.concatenate([np.arange(j[k], j[k] + d["nodes"][k]["len"]) for k in sub])
    got2 = eng.draws_predict(ids_of(mamba, m, sub), SEED, START, THIN)
    assert np.array_equal(got2, got[:, pick, :], equal_nan=True)
    sim = mamba.Chains(v, m.monitor_names, START, THIN, np.arange(1, v.shape[2] + 1), m, eng)
    assert sim.predict().names == ref.names(d, keys)


@pytest.mark.parametrize("name,m,mz", [("big300", 300, 150), ("big500", 500, 400)])   # tiles of 16 and of 8 chains
def test_large_state_tiles(mamba, monkeypatch, name, m, mz):
    v, d, keys, want, _ = fixture(name)
    z = tp.bigvec_draws(m)[0]
    M = tp.bigvec_short(mamba, m, mz, z)
    monkeypatch.setenv("MMB_IR_JIT", "0")
    eng = mamba.Engine(M)
    eng.init_chains(np.zeros((v.shape[2], m + 1)), seed=1)
    eng.set_draws(v)
    assert eng.predict_width([0]) == mz
    same(eng.draws_predict([0], SEED, START, THIN), want, d, keys)


# ---------------------------------------------------------------- invariance, bit for bit
def _full(mamba, monkeypatch, which):
    if which == "line":
        v = fixture("line")[0]
        m, eng = line_engine(mamba, v.shape[2])
        ids = [mamba.abi.MMB_LINE_Y]
    else:
        v, _, keys, _, _ = fixture("allfam")
        m, eng = allfam_engine(mamba, monkeypatch, v.shape[2])
        ids = ids_of(mamba, m, keys)
    eng.set_draws(v)
    return v, m, eng, ids


@pytest.mark.parametrize("which", ["line", "allfam"])
def test_invariance(mamba, monkeypatch, which):
    v, m, eng, ids = _full(mamba, monkeypatch, which)
    n, K = v.shape[0], v.shape[2]
    full = eng.draws_predict(ids, SEED, START, THIN)
    assert np.array_equal(eng.draws_predict(ids, SEED, START, THIN), full, equal_nan=True)       # the same call twice
    i0, i1 = (2, 5) if n >= 5 else (1, 3)
    assert np.array_equal(eng.draws_predict(ids, SEED, START, THIN, i0, i1), full[i0:i1], equal_nan=True)
    monkeypatch.setenv("MMB_PREDICT_CHUNK_ROWS", "2")            # a scratch of fewer rows than n
    assert np.array_equal(eng.draws_predict(ids, SEED, START, THIN), full, equal_nan=True)
    monkeypatch.delenv("MMB_PREDICT_CHUNK_ROWS")
    # two engines over the chain halves: global chain ids key the streams
    h = K // 2 + 1
    parts = []
    for off, sl in ((0, slice(0, h)), (h, slice(h, K))):
        if which == "line":
            mm = mamba.line()
            mm.setinputs(mamba.model.LINE_DATA)
            mm.setsamplers([mamba.AMWG(["beta", "s2"], 1.0)])
            e2 = mamba.Engine(mm)
            e2.init_chains(mamba.model.line_init_matrix(K, seed=3)[sl], chain_offset=off, seed=7)
        else:
            _, e2 = allfam_engine(mamba, monkeypatch, sl.stop - sl.start, off)
        e2.set_draws(v[:, :, sl])
        parts.append(e2.draws_predict(ids, SEED, START, THIN))
    assert np.array_equal(np.concatenate(parts, axis=2), full, equal_nan=True)
    assert not np.array_equal(eng.draws_predict(ids, SEED + 1, START, THIN), full, equal_nan=True)


@pytest.mark.parametrize("which", ["line", "allfam"])
def test_moments_are_the_row_order_sums(mamba, monkeypatch, which):
    v, m, eng, ids = _full(mamba, monkeypatch, which)
    yhat = eng.draws_predict(ids, SEED, START, THIN)
    rng = np.random.default_rng(4)
    shift = rng.normal(0.0, 1.0, yhat.shape[1])
    want = ref.moments(yhat, shift)
    assert np.array_equal(eng.draws_predict_moments(ids, SEED, START, THIN, shift), want, equal_nan=True)
    monkeypatch.setenv("MMB_PREDICT_CHUNK_ROWS", "2")            # continued over row chunks
    assert np.array_equal(eng.draws_predict_moments(ids, SEED, START, THIN, shift), want, equal_nan=True)
    assert np.isnan(want).any() and np.isfinite(want).any()     # non-finite values propagate, per (chain, column)


def _line_run(mamba, K, off=0, allK=64):
    m = mamba.line()
    m.setsamplers([mamba.AMWG(["beta", "s2"], 1.0)])
    init = mamba.model.line_init_matrix(allK, seed=5)[off:off + K]
    return mamba.mcmc(m, mamba.model.LINE_DATA, init, 400, burnin=200, chains=K, chain_offset=off, seed=11,
                      keep_device=True)


@pytest.fixture(scope="module")
def line_run(mamba):
    return _line_run(mamba, 64)


def test_predict_moments_sharded_over_two_engines(mamba, line_run):
    sim = line_run
    one, names, cols = sim.predict_summary()
    assert cols == ["Mean", "SD"] and names == [f"y[{i}]" for i in range(1, 6)] and one.shape == (5, 2)
    parts = [_line_run(mamba, 32, 0), _line_run(mamba, 32, 32)]
    assert np.array_equal(np.concatenate([p.value for p in parts], axis=2), sim.value)
    red = _SumOverRanks(2)
    out = [None, None]

    def rank(r):
        p = parts[r]
        out[r] = mamba.predict_moments_sharded(p.engine, p.model, None, red, None, p.start, p.thin)

    ts = [threading.Thread(target=rank, args=(r,), daemon=True) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert out[0] is not None and out[1] is not None
    np.testing.assert_allclose(out[0], one, rtol=1e-12)
    np.testing.assert_allclose(out[1], one, rtol=1e-12)


def test_end_to_end_on_sampler_output(mamba, line_run):
    """mcmc on line (64 chains, 200 kept), then predict: yhat_i = mu_i + sigma z with mu_i = beta1 + beta2 x_i
    of the same draw, so the pooled mean of yhat_i differs from the pooled mean of mu_i by the mean of
    N = 200 * 64 independent sigma z terms: Monte-Carlo standard error sqrt(mean(s2) / N), from the same draws."""
    sim = line_run
    assert sim.value.shape == (200, 3, 64)
    pp = sim.predict()
    assert pp.value.shape == (200, 5, 64) and pp.names == [f"y[{i}]" for i in range(1, 6)]
    assert pp.range == sim.range and np.array_equal(pp.chains, sim.chains) and np.isfinite(pp.value).all()
    summ, names, _ = sim.predict_summary()
    x = np.asarray(mamba.model.LINE_DATA["x"], float)
    for i in range(5):
        mu = sim.value[:, 0, :] + sim.value[:, 1, :] * x[i]
        se = np.sqrt(sim.value[:, 2, :].mean() / mu.size)
        assert abs(summ[i, 0] - mu.mean()) < 4.0 * se
        np.testing.assert_allclose(summ[i, 0], pp.value[:, i, :].mean(), rtol=1e-10)
        np.testing.assert_allclose(summ[i, 1], pp.value[:, i, :].std(ddof=1), rtol=1e-10)
        assert summ[i, 1] > np.sqrt(sim.value[:, 2, :].mean()) * 0.5


def test_nothing_is_disturbed(mamba):
    def fresh():
        m, eng = line_engine(mamba, 96)
        d = eng.run(60, burnin=20, thin=2, keep_device=True)
        return m, eng, d

    m, eng, d = fresh()
    _, twin, d2 = fresh()
    assert np.array_equal(d, d2)
    lo, hi = np.quantile(d[:, 0, :], [0.05, 0.95])
    nb, na = eng.hpd_collect(0, lo, hi, d[:, 0, :].size)
    before = (eng.values(), eng.tune(), eng.draws(), eng.iter, eng.chain_order(), *eng.hpd_get_tails(nb, na))
    sim = mamba.Chains(d, m.monitor_names, 22, 2, np.arange(1, 97), m, eng)
    sim.predict()
    sim.predict(rows=(3, 9))
    sim.predict_summary()
    after = (eng.values(), eng.tune(), eng.draws(), eng.iter, eng.chain_order(), *eng.hpd_get_tails(nb, na))
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert np.array_equal(eng.run(40, burnin=20, thin=2), twin.run(40, burnin=20, thin=2))
    assert np.array_equal(eng.values(), twin.values()) and np.array_equal(eng.tune(), twin.tune())


def test_refusals(mamba, monkeypatch):
    ir = mamba.ir
    Y = mamba.abi.MMB_LINE_Y
    ml, e0 = line_engine(mamba, 8)
    with pytest.raises(RuntimeError, match="call out of order"):      # no device-kept draws
        e0.draws_predict([Y], 1, 1, 1, 0, 1)
    with pytest.raises(RuntimeError, match="call out of order"):
        e0.draws_predict_moments([Y], 1, 1, 1, np.zeros(5))
    e0.set_draws(np.ones((4, 3, 8)))
    for nodes in ([mamba.abi.MMB_LINE_BETA], [mamba.abi.MMB_LINE_S2], [3], [Y, Y], []):   # not the output node
        with pytest.raises(RuntimeError, match="invalid argument"):
            e0.predict_width(nodes)
    for start, thin, i0, i1 in ((1, 0, 0, 4), (1, -1, 0, 4), (-1, 1, 0, 4), (1, 1, 2, 2), (1, 1, 3, 1), (1, 1, -1, 2),
                                (1, 1, 0, 5)):                         # thin = 0, start < 0, empty or outside windows
        with pytest.raises(RuntimeError, match="invalid argument"):
            e0.draws_predict([Y], 1, start, thin, i0, i1)
    with pytest.raises(RuntimeError, match="invalid argument"):
        e0.draws_predict_moments([Y], 1, 1, 0, np.zeros(5))
    sim = mamba.Chains(np.ones((4, 3, 8)), ml.monitor_names, 1, 1, np.arange(1, 9), ml, e0)
    with pytest.raises(mamba.ArgumentError, match="nodekeys are not all observed Stochastic nodess : y"):
        sim.predict("beta")
    with pytest.raises(mamba.ArgumentError, match="kept draws"):
        sim.predict(rows=(2, 2))

    # node IR: a sampled node, a Logical, an unmonitored parent (the message names it)
    m = ir.rats_model().setinputs(ir.rats_inputs())
    m.setsamplers(mamba.model.rats_scheme_reference())
    V = m.init_matrix(ir.rats_inits_ls(4, seed=2), 4)
    eng = ir_engine(mamba, monkeypatch, m, V)
    eng.set_draws(np.ones((2, 3, 4)))
    t = m.stats_table()["ids"]
    with pytest.raises(RuntimeError, match=f"node id {t['alpha']} is not monitored"):
        eng.draws_predict([t["y"]], 1, 1, 1)
    sim = mamba.Chains(np.ones((2, 3, 4)), m.monitor_names, 1, 1, np.arange(1, 5), m, eng)
    with pytest.raises(mamba.ArgumentError, match="alpha is not monitored"):
        sim.predict("y")
    with pytest.raises(mamba.ArgumentError, match="node alpha is not monitored"):
        mamba.modelstats._engine_call(m, eng.draws_predict, [t["y"]], 1, 1, 1)
    with pytest.raises(RuntimeError, match="not an observed Stochastic node"):
        eng.predict_width([t["mu_beta"]])                            # sampled, monitored
    with pytest.raises(RuntimeError, match="invalid argument"):
        eng.predict_width([list(m.order).index("alpha0")])           # a Logical
    with pytest.raises(RuntimeError, match="invalid argument"):
        eng.predict_width([len(m.order)])

    # the full-width 501-value model: (501 + 501) doubles per chain, not even 8 chains fit the 64 KiB
    z, v = tp.bigvec_draws(500)
    from test_gpu_modelstats import bigvec
    eb = mamba.Engine(bigvec(mamba, 500, z))
    eb.init_chains(np.zeros((9, 501)), seed=1)
    eb.set_draws(v)
    with pytest.raises(RuntimeError, match="unsupported"):
        eb.draws_predict([0], 1, 1, 1)

    r = mamba.rats()
    r.setinputs(mamba.model.RATS_DATA)
    r.setsamplers(mamba.model.rats_scheme_gibbs_amm())
    with pytest.raises(RuntimeError, match="unsupported"):
        mamba.Engine(r).predict_width([0])
    data, _ = mamba.model.logistic_data(64, 4)
    lg = mamba.logistic(64, 4)
    lg.setinputs(data)
    lg.setsamplers([mamba.NUTS("beta")])
    with pytest.raises(RuntimeError, match="unsupported"):
        mamba.Engine(lg).draws_predict_moments([0], 1, 1, 1, np.zeros(1))
