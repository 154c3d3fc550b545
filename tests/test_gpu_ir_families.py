"""Every node-IR family, link kind and support boundary on the device.

The element layer csrc/ir_math.h (ten families, four link kinds, lgamma) is shared by the
interpreter, the hipRTC-specialised kernels, modelstats.hip and the oracle, but the documentation
examples reach only Normal, MvNormal, InverseGamma, Gamma, Exponential, Binomial and Poisson and
the log link.  Here the all-family model zoo() of tests/test_ir.py (Beta, Uniform, Bernoulli; the
logit and affine-logit links; blocks that mix link kinds) runs under every sampler in both device
forms against the oracle, bit for bit; the element densities are evaluated by modelstats.hip at
and around every support boundary against the 50-digit reference tests/ir_family_ref.py; and the
wide-window Slice model whose boundary candidates were NaN (accepted by the shrink test) runs
NaN-free and equal to the oracle."""
import functools

import numpy as np
import pytest

import ir_family_ref as R
from test_gpu_ir import run_both
from test_gpu_rwm import check_exact, restate
from test_ir import ZOO_DATA, ZOO_FIXED, wide_slice, zoo, zoo_inits

pytestmark = pytest.mark.gpu

K = 33          # odd: the last wavefront holds one 32-lane group
I7 = 0.01 * np.eye(7)


def _mb():
    import _mamba_path
    return _mamba_path.load()


def zoo_model(mb, scheme, chains=K):
    """zoo() with the inits of test_ir_families_vs_scipy (default_rng(7), one dict per chain)."""
    m = zoo(mb).setinputs(ZOO_DATA).setsamplers(scheme)
    return m, m.init_matrix(zoo_inits(np.random.default_rng(7), chains), chains)


# Every scheme moves on the oracle with finite draws (asserted in the test); each specialised
# scheme compiles a kernel of its own, so the list stays this short.
SCHEMES = {
    "amwg": lambda M: [M.AMWG(["p", "a"], 0.1), M.AMWG(["lam", "g", "th"], 0.1), M.AMWG(["b", "m0"], 0.5)],
    "slice_tr": lambda M: [M.Slice(["p", "a"], 1.0, M.Univariate, transform=True),
                           M.Slice(["lam", "g", "th"], 1.0, transform=True), M.Slice(["b", "m0"], 1.0)],
    "slice_raw": lambda M: [M.Slice("p", 0.2, M.Univariate), M.Slice("a", 0.5), M.Slice("lam", 0.5, M.Univariate),
                            M.Slice(["g", "th"], 0.5, M.Multivariate), M.AMWG(["b", "m0"], 0.5)],
    "nuts": lambda M: [M.NUTS(["p", "a", "b"]), M.NUTS(["g", "th", "lam"]), M.AMWG("m0", 0.5)],
    "amm": lambda M: [M.AMM(["p", "a", "b", "m0"], I7), M.AMM(["lam", "g", "th"], I7)],
    "hmc_mala": lambda M: [M.HMC(["p", "a"], 0.05, 5), M.MALA(["lam", "g", "th"], 0.05), M.AMWG(["b", "m0"], 0.5)],
}
LANE_SCHEME = lambda M: [M.AMWG("p", 0.1), M.AMWG("lam", 0.1), M.AMWG(["a", "g", "th"], 0.1),     # noqa: E731
                         M.AMWG(["b", "m0"], 0.5)]
RWM_SCHEME = lambda M: [M.RWM(["p", "a"], 0.2, M.Cosine), M.RWM(["lam", "g", "th"], 0.2),         # noqa: E731
                        M.RWM(["b", "m0"], 0.5, M.SymUniform)]


LANE_NSEP = 2   # p and lam: the count the ir_jit() info string reports for LANE_SCHEME, pinned


def ir_models():
    """(label, model) of every node-IR model this file runs specialised (tools/jit_prebuild.py)."""
    mb = _mb()
    out = [(f"zoo_{k}", zoo_model(mb, s(mb), 2)[0]) for k, s in sorted(SCHEMES.items())]
    out.append(("zoo_lane_amwg", zoo_model(mb, LANE_SCHEME(mb), 2)[0]))
    out.append(("zoo_rwm", zoo_model(mb, RWM_SCHEME(mb), 2)[0]))
    out.append(("wide_slice", wide_slice(mb, 2)[0]))
    return out


# ---------------------------------------------------------------- 1. the zoo under every sampler
@pytest.mark.parametrize("kernel", ["specialised", "interpreter"])
@pytest.mark.parametrize("scheme", sorted(SCHEMES))
def test_zoo_gpu_vs_oracle(mamba, oracle, scheme, kernel, monkeypatch):
    """33 chains, 60 iterations, burn-in 20, thin 2: draws, values and tune rows of both device
    forms equal the oracle's, zero differing bits; the draws are finite and the chains move."""
    if kernel == "interpreter":
        monkeypatch.setenv("MMB_IR_JIT", "0")
    m, V = zoo_model(mamba, SCHEMES[scheme](mamba))
    eng, dg, st, do = run_both(mamba, oracle, m, V, 60, 20, 2, jit=kernel == "specialised")
    # not vacuous (on the oracle's draws; the comparison below is the check): most (column, chain)
    # series change at least once over the 20 kept draws -- all of them in five schemes, 65 % under
    # nuts, whose second block is stuck in some chains.  This counts series, not steps.
    assert np.isfinite(do).all() and (np.ptp(do, axis=0) > 0).mean() > 0.6
    np.testing.assert_array_equal(dg, do)
    np.testing.assert_array_equal(eng.values(), st["values"])
    np.testing.assert_array_equal(eng.tune(), st["tune"][:, :st["tl"]])


def test_zoo_lane_parallel_amwg(mamba, oracle, monkeypatch):
    """p and lam alone separate by coordinate (each Binomial, Bernoulli, Poisson, Beta or Gamma
    element reads one of the block's coordinates): the specialised kernel decides their coordinates
    at once.  The three modes of test_ir_lane_parallel_amwg equal the oracle bit for bit and the
    sequential fallback stays within 1 % of the lane-parallel blocks' updates."""
    m, V = zoo_model(mamba, LANE_SCHEME(mamba))
    nsep = LANE_NSEP
    out, seq = {}, {}
    for mode in ("sep", "sequential", "wide"):
        monkeypatch.setenv("MMB_IR_SEP", "0" if mode == "sequential" else "1")
        monkeypatch.setenv("MMB_AMWG_EXACT", "2" if mode == "wide" else "0")
        eng = mamba.Engine(m)
        jit, info = eng.ir_jit()
        assert jit, info
        if mode != "sequential":
            assert f"lane-parallel AMWG blocks: {nsep} of" in info, info
        eng.init_chains(V, seed=23)
        d = eng.run(80, burnin=20, thin=2)
        out[mode] = (d, eng.values(), eng.tune())
        seq[mode] = eng.amwg_stats()["sequential_updates"]
    st = oracle.new_state(m, V)
    do = oracle.run(m, st, 80, burnin=20, thin=2, seed=23, nthreads=8)
    for mode in out:
        np.testing.assert_array_equal(out[mode][0], do)
        np.testing.assert_array_equal(out[mode][1], st["values"])
        np.testing.assert_array_equal(out[mode][2], st["tune"][:, :st["tl"]])
    updates = nsep * V.shape[0] * 80
    print("sequential updates", seq, "of", updates)
    assert seq["sep"] <= 0.01 * updates, (seq, updates)
    assert seq["wide"] > seq["sep"], seq


@functools.lru_cache(maxsize=None)
def rwm_zoo_ref():
    mb = _mb()
    return restate(lambda sch: zoo_model(mb, sch), RWM_SCHEME(mb), 11, 60, 20, 2)


@pytest.mark.parametrize("kernel", ["specialised", "interpreter"])
def test_zoo_rwm_exact(mamba, kernel, monkeypatch):
    """RWM blocks through the logit (p), affine-logit (a) and log links, Cosine, Normal and SymUniform
    proposals, against the Python restatement tests/rwm_ref.py (the oracle has no RWM): draws,
    values, tune rows and update / accept counts identical.  Not vacuous: every block accepts
    between 10 % and 95 % of its updates."""
    if kernel == "interpreter":
        monkeypatch.setenv("MMB_IR_JIT", "0")
    ref = rwm_zoo_ref()
    for b, v in ref[3].items():
        assert 0.10 <= v["accepts"] / v["updates"] <= 0.95, (b, v)
    m, V = zoo_model(mamba, RWM_SCHEME(mamba))
    eng = mamba.Engine(m)
    assert eng.ir_jit()[0] == (kernel == "specialised"), eng.ir_jit()
    eng.init_chains(V, seed=11)
    dg = eng.run(60, burnin=20, thin=2)
    check_exact(eng, dg, ref)
    eng.close()


# ---------------------------------------------------------------- 2. element densities at the edges
def _upload(mamba, monkeypatch, m, V, base, cells):
    """One (row, chain) cell per grid point: the draws buffer n x pmon x K with `base` everywhere and
    each cell's overrides; returns the engine (interpreter: modelstats.hip runs its code) and the
    cell -> (row, chain) map."""
    monkeypatch.setenv("MMB_IR_JIT", "0")
    eng = mamba.Engine(m)
    eng.init_chains(V, seed=1)
    col = {n: j for j, n in enumerate(m.monitor_names)}
    assert set(base) == set(col), (sorted(base), sorted(col))
    n = -(-len(cells) // K)
    v = np.empty((n, len(col), K))
    for name, val in base.items():
        v[:, col[name], :] = val
    for c, (_, over, _) in enumerate(cells):
        for name, val in over.items():
            v[c // K, col[name], c % K] = val
    eng.set_draws(v)
    return eng


def _check_cells(mamba, m, eng, cells):
    got = {}
    bad = []
    worst = {}
    for c, (key, over, want) in enumerate(cells):
        if key not in got:
            got[key] = eng.draws_logpdf(mamba.modelstats.node_ids(m, [key]))
        g = float(got[key][c // K, c % K])
        try:
            e = R.check(g, want[0], want[1], where=(key, over))
            if want[1] > 0:
                worst[key] = max(worst.get(key, 0.0), e / (1e-12 * want[1] + 1e-13))
        except AssertionError as ex:
            bad.append(str(ex))
    print("cells", len(cells), "worst error / bound per node", worst)
    assert not bad, f"{len(bad)} of {len(cells)} cells:\n" + "\n".join(bad[:40])


def zoo_cells():
    cells = []
    for i, (x, a, b) in enumerate(R.edge_grid("beta")):          # p ~ Beta(a, b): the probe in element i % 4
        parts = [R.logpdf("beta", x if e == i % 4 else 0.5, a, b) for e in range(4)]
        cells.append(("p", {f"p[{i % 4 + 1}]": x, "a": a, "b": b}, R.total(parts)))
    for i, (x, a, b) in enumerate(R.edge_grid("gamma")):         # lam ~ Gamma(g, th)
        parts = [R.logpdf("gamma", x if e == i % 5 else 1.0, a, b) for e in range(5)]
        cells.append(("lam", {f"lam[{i % 5 + 1}]": x, "g": a, "th": b}, R.total(parts)))
    ks, ns = ZOO_FIXED["obs_bin"], ZOO_DATA["nn"]               # k = 3 of 10, 0 of 12, 7 of 7, 11 of 20
    for j in range(4):
        for p in R.PROBS:
            parts = [R.logpdf("binomial", ks[e], ns[e], p if e == j else 0.5) for e in range(4)]
            cells.append(("obs_bin", {f"p[{j + 1}]": p}, R.total(parts)))
    kp, t = ZOO_FIXED["obs_poi"], ZOO_DATA["t"]                 # k = 0, 4, 1, 9, 2
    for j in (0, 1, 3):
        for lam in R.RATES:
            parts = [R.logpdf("poisson", kp[e], (lam if e == j else 1.0) * t[e]) for e in range(5)]
            cells.append(("obs_poi", {f"lam[{j + 1}]": lam}, R.total(parts)))
    for p in R.PROBS:                                           # obs_ber = 1, 0, 1 ~ Bernoulli(p[1])
        cells.append(("obs_ber", {"p[1]": p}, R.total([R.logpdf("bernoulli", x, p) for x in ZOO_FIXED["obs_ber"]])))
    for x, _, _ in R.edge_grid("uniform"):                      # a ~ Uniform(0.5, 4)
        cells.append(("a", {"a": x}, R.logpdf("uniform", x, lo=R.UNIFORM_LO, hi=R.UNIFORM_HI)))
    return cells


def test_zoo_edge_densities(mamba, monkeypatch):
    """Beta, Gamma, Binomial, Poisson, Bernoulli and Uniform elements through modelstats.hip
    (set_draws, draws_logpdf: the sweep kernel's interpreter on caller-supplied values) at every
    point of the edge grid: the class (nan, +inf, -inf, finite) is the reference's and a finite
    value lies within 1e-12 M + 1e-13 of it (1e-12: the project's rtol for log densities, applied
    to the term scale M so that cancellation is priced in)."""
    m, V = zoo_model(mamba, SCHEMES["amwg"](mamba))
    base = {**{f"p[{i}]": 0.5 for i in range(1, 5)}, **{f"lam[{i}]": 1.0 for i in range(1, 6)},
            "g": 1.0, "th": 1.0, "a": 1.0, "b": 1.0, "m0": 3.0}
    cells = zoo_cells()
    assert 500 < len(cells) < 700
    eng = _upload(mamba, monkeypatch, m, V, base, cells)
    _check_cells(mamba, m, eng, cells)


def params_model(mamba):
    """InverseGamma, Exponential and Normal nodes whose parameters are nodes too, so a draw sets them."""
    ir = mamba.ir
    m = ir.Model(
        s=ir.Stochastic(1, lambda ia, ib: ir.InverseGamma(ia, ib)),
        e=ir.Stochastic(lambda es: ir.Exponential(es)),
        z=ir.Stochastic(lambda mu, sd: ir.Normal(mu, sd)),
        ia=ir.Stochastic(lambda: ir.Gamma(2.0, 1.0)), ib=ir.Stochastic(lambda: ir.Gamma(2.0, 1.0)),
        es=ir.Stochastic(lambda: ir.Gamma(2.0, 1.0)), mu=ir.Stochastic(lambda: ir.Normal(0.0, 10.0)),
        sd=ir.Stochastic(lambda: ir.Gamma(2.0, 1.0)))
    m.setinputs({})
    m.setsamplers([mamba.AMWG(["s", "e", "z"], 0.1), mamba.AMWG(["ia", "ib", "es"], 0.1), mamba.AMWG(["mu", "sd"], 0.1)])
    init = {"s": [1.0, 1.0, 1.0], "e": 1.0, "z": 0.0, "ia": 1.0, "ib": 1.0, "es": 1.0, "mu": 0.0, "sd": 1.0}
    return m, m.init_matrix([init] * K, K)


def params_cells():
    cells = []
    for i, (x, a, b) in enumerate(R.edge_grid("invgamma")):
        parts = [R.logpdf("invgamma", x if e == i % 3 else 1.0, a, b) for e in range(3)]
        cells.append(("s", {f"s[{i % 3 + 1}]": x, "ia": a, "ib": b}, R.total(parts)))
    for x, a, _ in R.edge_grid("exponential"):
        cells.append(("e", {"e": x, "es": a}, R.logpdf("exponential", x, a)))
    for x, a, b in R.edge_grid("normal"):
        cells.append(("z", {"z": x, "mu": a, "sd": b}, R.logpdf("normal", x, a, b)))
    return cells


def test_params_edge_densities(mamba, monkeypatch):
    """InverseGamma, Exponential and Normal elements at the edge grid, as test_zoo_edge_densities."""
    m, V = params_model(mamba)
    base = {"s[1]": 1.0, "s[2]": 1.0, "s[3]": 1.0, "e": 1.0, "z": 0.0, "ia": 1.0, "ib": 1.0, "es": 1.0, "mu": 0.0,
            "sd": 1.0}
    cells = params_cells()
    assert 300 < len(cells) < 450
    eng = _upload(mamba, monkeypatch, m, V, base, cells)
    _check_cells(mamba, m, eng, cells)


# ---------------------------------------------------------------- 3. the wide-window Slice model
@pytest.mark.parametrize("kernel", ["specialised", "interpreter"])
def test_wide_slice_gpu_vs_oracle(mamba, oracle, kernel, monkeypatch):
    """test_ir.py's wide-window Slice model (Beta(1, 1) and Gamma(1, 2) priors, windows of 100 and
    3000 on the link scale), 33 chains, 40 iterations, every one kept: candidates at p = 0 or 1,
    lam = 0 or Inf have log density -Inf on the device as on the oracle, so the draws are
    NaN-free, inside the supports, and equal bit for bit."""
    if kernel == "interpreter":
        monkeypatch.setenv("MMB_IR_JIT", "0")
    m, V = wide_slice(mamba, K)
    eng, dg, st, do = run_both(mamba, oracle, m, V, 40, 0, 1, seed=17, jit=kernel == "specialised")
    assert np.isfinite(dg).all(), int((~np.isfinite(dg)).sum())
    assert (dg > 0).all() and (dg[:, :4, :] < 1).all()
    np.testing.assert_array_equal(dg, do)
    np.testing.assert_array_equal(eng.values(), st["values"])
