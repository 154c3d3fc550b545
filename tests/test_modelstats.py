"""Model statistics on the host (mamba.jl_amd/modelstats.py, Model.keys) without a GPU: the
restatement tests/modelstats_ref.py against scipy.stats, dic_sharded's closing formulas and its
sharding against the restatement through an engine-shaped fake, the node tables of the models and
the argument errors."""
import math
import threading

import numpy as np
import pytest
from scipy import stats

import modelstats_ref as ref


def line_draws(n=37, K=70, seed=7):
    """n x 3 x K: beta1 ~ N(0.6, 1), beta2 ~ N(0.8, 0.3), s2 = exp(N(0, 0.5))."""
    rng = np.random.default_rng(seed)
    v = np.empty((n, 3, K))
    v[:, 0, :] = rng.normal(0.6, 1.0, (n, K))
    v[:, 1, :] = rng.normal(0.8, 0.3, (n, K))
    v[:, 2, :] = np.exp(rng.normal(0.0, 0.5, (n, K)))
    return v


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def test_restated_densities_equal_scipy():
    v = line_draws()
    for i, k in [(0, 0), (5, 11), (36, 69), (17, 33)]:
        b0, b1, s2 = v[i, :, k]
        sig = math.sqrt(s2)
        assert rel(ref.normal_lp(b0, 0.3, sig), stats.norm.logpdf(b0, 0.3, sig)) < 1e-12
        mu = b0 + b1 * ref.LINE_X
        assert rel(ref.iso_normal_lp(ref.LINE_Y, mu, sig), stats.norm.logpdf(ref.LINE_Y, mu, sig).sum()) < 1e-12
        assert rel(ref.normal_vec_lp(ref.LINE_Y, mu, sig), stats.norm.logpdf(ref.LINE_Y, mu, sig).sum()) < 1e-12
        assert rel(ref.iso_normal_lp([b0, b1], 0.0, math.sqrt(1000.0)),
                   stats.norm.logpdf([b0, b1], 0.0, math.sqrt(1000.0)).sum()) < 1e-12
        assert rel(ref.invgamma_lp(s2, 0.001, 0.001), stats.invgamma.logpdf(s2, 0.001, scale=0.001)) < 1e-12
        assert rel(ref.invgamma_lp(s2, 2.5, 1.5), stats.invgamma.logpdf(s2, 2.5, scale=1.5)) < 1e-12
    r = [10, 23, 0, 3, 7]
    n = [39, 62, 4, 12, 7]
    p = ref.invlogit(np.array([-0.5, 0.1, -1.0, 0.3, 2.0]))
    for a, b, c in zip(r, n, p):
        assert rel(ref.binomial_lp(a, b, c), stats.binom.logpmf(a, b, c)) < 1e-12
    assert ref.invgamma_lp(-1.0, 0.001, 0.001) == -math.inf
    assert ref.iso_normal_lp([1.0, math.inf], 0.0, 1.0) == -math.inf


def _line_fake(mamba, value):
    ids = mamba.line().stats_table()["ids"]
    return ref.FakeEngine(value, ref.line_desc(), {v: k for k, v in ids.items()})


def test_dic_sharded_equals_restatement(mamba):
    v = line_draws()
    got, rows, cols = mamba.dic_sharded(_line_fake(mamba, v), mamba.line())
    want, _ = ref.dic(v, ref.line_desc(), ["y"])
    assert rows == ["pD", "pV"] and cols == ["DIC", "Effective Parameters"]
    assert got.shape == (2, 2)
    np.testing.assert_allclose(got, want, rtol=1e-12)
    # no cancellation in the variance for this input: S2 / (S2 - S1^2 / N) stays small
    D = -2.0 * ref.logpdf_draws(v, ref.line_desc(), ["y"]) - ref.dic(v, ref.line_desc(), ["y"])[1]
    S1, S2, N = D.sum(), (D * D).sum(), D.size
    assert S2 / (S2 - S1 * S1 / N) < 2.0


class _SumOverRanks:
    """A summing all-reduce over `n` threads of one process."""

    def __init__(self, n):
        self.bar = threading.Barrier(n, timeout=20)
        self.lock = threading.Lock()
        self.parts = []

    def __call__(self, v):
        with self.lock:
            self.parts.append(np.asarray(v, dtype=np.float64))
        self.bar.wait()
        tot = np.sum(self.parts, axis=0)
        self.bar.wait()
        with self.lock:
            self.parts = []
        self.bar.wait()
        return tot


def test_dic_sharded_over_two_shards(mamba):
    v = line_draws()
    single = mamba.dic_sharded(_line_fake(mamba, v), mamba.line())[0]
    red = _SumOverRanks(2)
    out = [None, None]

    def rank(r, part):
        out[r] = mamba.dic_sharded(_line_fake(mamba, part), mamba.line(), allreduce_sum=red)[0]

    ts = [threading.Thread(target=rank, args=(r, part), daemon=True)
          for r, part in enumerate((v[:, :, :31], v[:, :, 31:]))]
    for t in ts:
        t.start()
    for t in ts:
        t.join(60)
    assert out[0] is not None and out[1] is not None
    np.testing.assert_allclose(out[0], single, rtol=1e-12)
    np.testing.assert_allclose(out[1], single, rtol=1e-12)


def _ir(mamba, name):
    ir = mamba.ir
    if name == "line":
        m = ir.line_model().setinputs(mamba.model.LINE_DATA)
        m.setsamplers([mamba.AMWG(["beta", "s2"], 1.0)])
        m.init_matrix([{"y": [1.0, 3, 3, 3, 5], "beta": [0.0, 0.0], "s2": 1.0}], 1)
    elif name == "seeds":
        m = ir.seeds_model().setinputs(ir.SEEDS)
        m.setsamplers([mamba.AMM(["alpha0", "alpha1", "alpha2", "alpha12"], 0.01 * np.eye(4)),
                       mamba.AMWG("b", 0.01), mamba.AMWG("s2", 0.1)])
        m.init_matrix(ir.seeds_inits(), 2)
    else:
        m = ir.rats_model().setinputs(ir.rats_inputs())
        m.setsamplers(ir.rats_scheme_gibbs_amm() if name == "rats_gibbs" else mamba.model.rats_scheme_reference())
        m.init_matrix(ir.rats_inits_ls(2), 2)
    return m


def test_keys(mamba):
    m = mamba.line()
    assert m.keys("output") == ["y"]
    assert m.keys("stochastic") == ["y", "beta", "s2"]
    m = _ir(mamba, "line")
    assert m.keys("output") == ["y"]
    assert m.keys("stochastic") == ["y", "beta", "s2"]
    m = _ir(mamba, "seeds")
    assert m.keys("output") == ["r"]
    assert m.keys("stochastic") == ["r", "b", "alpha0", "alpha1", "alpha2", "alpha12", "s2"]
    for name in ("rats", "rats_gibbs"):  # a Gibbs closure that reads y does not make y a parent
        m = _ir(mamba, name)
        assert m.keys("output") == ["y"]
        assert m.keys("stochastic") == ["y", "alpha", "mu_alpha", "s2_alpha", "beta", "mu_beta", "s2_beta", "s2_c"]
    with pytest.raises(mamba.ArgumentError):
        m.keys("block")
    with pytest.raises(mamba.ArgumentError):
        mamba.ir.rats_model().keys("output")   # not lowered yet: node lengths unknown


def test_needed_nodes(mamba):
    need = mamba.modelstats.needed_nodes
    m = _ir(mamba, "rats")
    assert need(m, "y") == ["alpha", "beta", "s2_c"]
    assert need(m, ["alpha"]) == ["alpha", "mu_alpha", "s2_alpha"]
    assert need(m, ["mu_beta"]) == ["mu_beta"]
    assert need(m, None) == ["alpha", "mu_alpha", "s2_alpha", "beta", "mu_beta", "s2_beta", "s2_c"]
    m = _ir(mamba, "seeds")
    assert need(m, "r") == ["b", "alpha0", "alpha1", "alpha2", "alpha12"]
    assert need(m, "b") == ["b", "s2"]
    m = _ir(mamba, "line")
    assert need(m, "y") == ["beta", "s2"]   # through the Logical mu
    assert need(mamba.line(), ["s2"]) == ["s2"]
    ids = mamba.modelstats.node_ids(mamba.line(), ["beta", "s2", "y"])
    assert ids.dtype == np.int32 and list(ids) == [0, 1, 2]


def test_argument_errors(mamba):
    ids = mamba.modelstats.node_ids
    with pytest.raises(mamba.ArgumentError, match="alpha"):
        ids(_ir(mamba, "rats"), "y")                 # alpha, beta are not monitored in the shipped model
    with pytest.raises(mamba.ArgumentError, match="b is not monitored"):
        ids(_ir(mamba, "seeds"), ["r"])
    with pytest.raises(mamba.ArgumentError, match="nu"):
        ids(mamba.line(), ["y", "nu"])
    with pytest.raises(mamba.ArgumentError, match="alpha"):
        ids(mamba.rats(), ["y"])                     # hand-lowered rats: 3 of 65 values monitored
    with pytest.raises(mamba.ArgumentError):
        mamba.dic_sharded(_line_fake(mamba, line_draws(3, 2)), mamba.rats())
    sim = mamba.Chains(line_draws(3, 2), ["beta[1]", "beta[2]", "s2"], 1, 1, [1, 2], mamba.line(), None)
    with pytest.raises(mamba.ArgumentError):
        sim.logpdf("nu")
    with pytest.raises(mamba.ArgumentError):
        sim.dic()                                    # no device-kept draws
    with pytest.raises(mamba.ArgumentError):
        mamba.logpdf(sim)
