"""DGS blocks on the device against the plain-Python restatement (tests/dgs_ref.py).

Replay checks are decision-exact away from thresholds: every chosen value equals the restatement's,
except where u lies within dgs_ref.DELTA of one of its cumulative probabilities (at most 2 such updates
per test; tests/test_dgs.py shows the restatement alone meets none on these seeds).  All runs: thin 1,
burnin 0, every sampled node monitored.
"""
import functools
import itertools
import math

import numpy as np
import pytest

import dgs_ref

pytestmark = pytest.mark.gpu
SEED = 11


def _mb():
    import _mamba_path
    return _mamba_path.load()


def _uniform():
    import oracle_lib
    return oracle_lib.Oracle().L.orc_uniform


SCHEMES = {
    "model1": lambda mb: [mb.DGS("z")],
    "model2": lambda mb: [mb.DGS("T")],
    "model3": lambda mb: [mb.DGS("T"), mb.RWM("mu", 0.3)],
    "model3r": lambda mb: [mb.RWM("mu", 0.3), mb.DGS("T")],
    "model4": lambda mb: [mb.DGS(["k", "tau"])],
    "model5": lambda mb: [mb.DGS("z")],
}


def build(name, K):
    mb = _mb()
    m, inputs, inits = getattr(dgs_ref, name.rstrip("r"))(mb.ir)
    m.setinputs(inputs).setsamplers(SCHEMES[name](mb))
    return m, m.init_matrix(inits(K), K)


def run(name, K, iters, chain_offset=0, windows=None, init=None):
    """(draws [iters, pmon, K], init matrix, jit info) of one engine; `windows` splits the run."""
    mb = _mb()
    m, V = build(name, K)
    if init is not None:
        V = init
    eng = mb.Engine(m)
    eng.init_chains(V, chain_offset=chain_offset, seed=SEED)
    d = np.concatenate([eng.run(w) for w in (windows or [iters])], axis=0)
    info = eng.ir_jit()
    eng.close()
    return d, V, info


@functools.lru_cache(maxsize=None)
def cached(name, K, iters):
    return run(name, K, iters)


def replay(name, spec, K, iters):
    d, V, _ = cached(name, K, iters)
    R = dgs_ref.Replay(_uniform(), spec, SEED).run(V, d)
    print(f"{name}: {R.updates} updates, {R.skips} threshold skips, {len(R.mismatch)} mismatches")
    assert R.mismatch == []
    assert R.skips <= 2
    return R


# ---- 1. Bernoulli with a data-index gather
def test_bernoulli_replay():
    R = replay("model1", dgs_ref.spec1(), 8, 200)
    assert R.updates == 8 * 200 * 3


def test_bernoulli_exact_posterior():
    """4096 independent chains, 30 sweeps, the last one only: the pooled frequencies of the 8 states
    against the enumerated posterior within 5 standard errors sqrt(p (1 - p) / 4096)."""
    K = 4096
    mb = _mb()
    m, V = build("model1", K)
    eng = mb.Engine(m)
    eng.init_chains(V, seed=SEED)
    d = eng.run(30, burnin=29)
    eng.close()
    assert d.shape == (1, 3, K)
    states = list(itertools.product([0, 1], repeat=3))
    lp = [dgs_ref.model1_lp(z) for z in states]
    mx = max(lp)
    w = [math.exp(x - mx) for x in lp]
    post = [x / math.fsum(w) for x in w]
    code = (d[0, 0] * 4 + d[0, 1] * 2 + d[0, 2]).astype(int)
    freq = np.bincount(code, minlength=8) / K
    for s, (p, f) in enumerate(zip(post, freq)):
        se = math.sqrt(p * (1.0 - p) / K)
        print(f"state {states[s]}: posterior {p:.5f}, frequency {f:.5f}, {abs(f - p) / se:.2f} se")
    for p, f in zip(post, freq):
        assert abs(f - p) <= 5.0 * math.sqrt(p * (1.0 - p) / K)


# ---- 2. Categorical longer than a lane group, a data vector gathered by the state (DATAV)
def test_categorical_replay():
    R = replay("model2", dgs_ref.spec2(), 4, 200)
    assert R.updates == 4 * 200 * 40


# ---- 3. a sampled vector gathered by the state (VALV), DGS mixed with RWM in both orders
@pytest.mark.parametrize("name,first", [("model3", True), ("model3r", False)])
def test_mixed_scheme_replay(name, first):
    d, _, _ = cached(name, 4, 200)
    assert len(np.unique(d[:, 40:, :])) > 100  # mu moves: the DGS conditionals see a changing mu
    replay(name, dgs_ref.spec3(first), 4, 200)


# ---- 4. Binomial with per-element supports and DiscreteUniform, one DGS over both keys
def test_binomial_discreteuniform_replay():
    R = replay("model4", dgs_ref.spec4(), 8, 200)
    assert R.updates == 8 * 200 * 5
    d, _, _ = cached("model4", 8, 200)
    assert d[:, 0].max() <= 3 and d[:, 1].max() <= 5 and d[:, :2].min() >= 0
    assert d[:, 2:].min() >= 1 and d[:, 2:].max() <= 10


# ---- 5. psum = 0: the uniform 1 / n inversion, exact
def test_zero_mass_branch():
    R = replay("model5", dgs_ref.spec5(), 8, 200)
    assert R.skips == 0
    d, _, _ = cached("model5", 8, 200)
    u = _uniform()
    want = np.array([[0.0 if u(SEED, c, t + 1, 0, dgs_ref.SUB_UNIFORM, 0) < 0.5 else 1.0 for c in range(8)]
                     for t in range(200)])
    np.testing.assert_array_equal(d[:, 0, :], want)


# ---- 6. stream hygiene
def test_windows_and_chain_offset():
    d, V, _ = cached("model3", 4, 200)
    d2, _, _ = run("model3", 4, 200, windows=[77, 123])
    np.testing.assert_array_equal(d2, d)
    da, _, _ = run("model3", 1, 200, init=V[:1])
    db, _, _ = run("model3", 3, 200, chain_offset=1, init=V[1:])
    np.testing.assert_array_equal(np.concatenate([da, db], axis=2), d)


# ---- 7. interpreter against the default kernel selection
@pytest.mark.parametrize("name", ["model2", "model3"])
def test_interpreter_vs_default(name, monkeypatch):
    d, V, (jit, info) = cached(name, 4, 200)
    # the specialised kernel generates no DGS code: it declines, says why, and the interpreter runs
    assert not jit and "DGS" in info, info
    monkeypatch.setenv("MMB_IR_JIT", "0")
    d0, _, (jit0, info0) = run(name, 4, 200)
    assert not jit0 and "MMB_IR_JIT=0" in info0
    np.testing.assert_array_equal(d0, d)


# ---- 8. model statistics on a model with DGS blocks
def test_logpdf_dic_predict():
    mb = _mb()
    m, inputs, inits = dgs_ref.model2(mb.ir)
    m.setsamplers([mb.DGS("T")])
    K, n = 4, 50
    sim = mb.mcmc(m, inputs, inits(K), n, chains=K, seed=SEED, keep_device=True)
    assert sim.value.shape == (n, 40, K)
    lp = sim.logpdf(["T", "y"]).value
    worst = 0.0
    for i in range(n):
        for k in range(K):
            want, mag = dgs_ref.model2_logpdf(sim.value[i, :, k])
            worst = max(worst, abs(lp[i, 0, k] - want) / mag)
            assert abs(lp[i, 0, k] - want) <= 1e-12 * mag
    print(f"logpdf: worst error {worst:.2e} of the sum of absolute terms")
    # the deviance at the posterior mean of a discrete node is undefined: refused, not garbage
    with pytest.raises(mb.ArgumentError, match="discrete node"):
        sim.dic()
    # predict(y): mu[T] + s z on the draw's own T, z = normal #e of the node's predict stream
    import oracle_lib
    L = oracle_lib.Oracle().L
    yh = sim.predict(["y"]).value
    nid = m.order.index("y")
    for i in (0, n - 1):
        for k in range(K):
            for e in (0, 17, 39):
                z = L.orc_normal(SEED, k, sim.start + i * sim.thin, 256 + nid, 0, e)
                assert yh[i, e, k] == dgs_ref.M2_MU[int(sim.value[i, e, k]) - 1] + dgs_ref.M2_S * z
