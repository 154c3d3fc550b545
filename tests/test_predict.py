"""Posterior prediction on the host, without a GPU: the restatement tests/predict_ref.py against the
exact distributions, its edge cases, the host logic of mamba.jl_amd/modelstats.py (names, default
keys, argument errors, the rows window) through an engine-shaped fake, and the fixtures the GPU
tests compare against (tests/test_gpu_predict.py imports them from here, computed once).

Goodness of fit, fixed seeds (deterministic: the p-values below are what these runs give).
chi-square on cells of expected count >= 5 (tails pooled):
    Bernoulli(0.3) 0.6788   Binomial(81, 0.3) 0.4623   Binomial(81, 0.8) 0.7409
    Binomial(1300, 0.45) 0.1555   Binomial(1300, 0.62) 0.1336   Poisson(3) 0.3782   Poisson(700) 0.2886
Kolmogorov-Smirnov against scipy.stats:
    Normal(0.3, 1.7) 0.5420   Exponential(2.5) 0.7516   Uniform(-1, 3) 0.9543   Gamma(0.4, 2) 0.7769
    Gamma(3.5, 0.7) 0.4007   InverseGamma(2.5, 1.5) 0.4667   Beta(0.5, 2) 0.2059   Beta(3, 4) 0.8778
Every one is asserted to be above 1e-3.
"""
import functools
import math

import numpy as np
import pytest
from scipy import stats

import modelstats_ref as mref
import predict_ref as ref
from test_modelstats import line_draws

NAN, INF = float("nan"), float("inf")


@functools.lru_cache(maxsize=None)
def lib():
    import oracle_lib
    return oracle_lib.Oracle().L


# ---------------------------------------------------------------- the restatement against the distributions
def chi2_p(x, dist, lo, hi):
    """Cells lo .. hi plus the two tails, merged from the ends until every expectation is >= 5."""
    x = np.asarray(x)
    ks = np.arange(lo, hi + 1)
    obs = np.concatenate([[np.sum(x < lo)], [np.sum(x == k) for k in ks], [np.sum(x > hi)]]).astype(float)
    exp = np.concatenate([[dist.cdf(lo - 1)], dist.pmf(ks), [dist.sf(hi)]]) * x.size
    o, e = list(obs), list(exp)
    while len(e) > 2 and e[0] < 5:
        e[1] += e[0]; o[1] += o[0]; e.pop(0); o.pop(0)       # noqa: E702
    while len(e) > 2 and e[-1] < 5:
        e[-2] += e[-1]; o[-2] += o[-1]; e.pop(); o.pop()     # noqa: E702
    return stats.chisquare(o, np.asarray(e) * (np.sum(o) / np.sum(e))).pvalue


DISCRETE_CASES = [  # family, a, b, count, seed, scipy distribution, cell range
    ("bernoulli", 0.3, 0.0, 4000, 1, stats.bernoulli(0.3), (0, 1)),
    ("binomial", 81.0, 0.3, 3000, 2, stats.binom(81, 0.3), (10, 40)),
    ("binomial", 81.0, 0.8, 3000, 3, stats.binom(81, 0.8), (50, 78)),
    ("binomial", 1300.0, 0.45, 2000, 4, stats.binom(1300, 0.45), (530, 640)),
    ("binomial", 1300.0, 0.62, 2000, 5, stats.binom(1300, 0.62), (750, 860)),
    ("poisson", 3.0, 0.0, 4000, 26, stats.poisson(3.0), (0, 12)),
    ("poisson", 700.0, 0.0, 2000, 7, stats.poisson(700.0), (620, 780)),
]
CONTINUOUS_CASES = [
    ("normal", 0.3, 1.7, 4000, 11, stats.norm(0.3, 1.7)),
    ("exponential", 2.5, 0.0, 4000, 12, stats.expon(scale=2.5)),
    ("uniform", -1.0, 3.0, 4000, 13, stats.uniform(-1.0, 4.0)),
    ("gamma", 0.4, 2.0, 3000, 14, stats.gamma(0.4, scale=2.0)),
    ("gamma", 3.5, 0.7, 3000, 15, stats.gamma(3.5, scale=0.7)),
    ("invgamma", 2.5, 1.5, 3000, 16, stats.invgamma(2.5, scale=1.5)),
    ("beta", 0.5, 2.0, 3000, 17, stats.beta(0.5, 2.0)),
    ("beta", 3.0, 4.0, 3000, 18, stats.beta(3.0, 4.0)),
]


@pytest.mark.parametrize("case", DISCRETE_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_discrete_families_fit(case):
    fam, a, b, count, seed, dist, (lo, hi) = case
    x = ref.variates(lib(), fam, a, b, count, seed=seed, n=3)
    assert np.all(x == np.round(x)) and x.min() >= 0
    p = chi2_p(x, dist, lo, hi)
    print(fam, a, b, "chi-square p =", round(float(p), 4))
    assert p > 1e-3


@pytest.mark.parametrize("case", CONTINUOUS_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_continuous_families_fit(case):
    fam, a, b, count, seed, dist = case
    x = ref.variates(lib(), fam, a, b, count, seed=seed, n=3)
    p = stats.kstest(x, dist.cdf).pvalue
    print(fam, a, b, "KS p =", round(float(p), 4))
    assert p > 1e-3


def test_binomial_chunks_and_poisson_pieces_use_their_own_uniforms():
    """n = 1300 is chunks of 512, 512 and 276 on uniforms #e, #(len + e), #(2 len + e): the sum of the
    three chunk draws made one by one on those uniforms."""
    L, key = lib(), (9, 4, 6, ref.pb(2))
    length, e, p = 7, 3, 0.45
    whole = ref.binomial(L, key, 1300.0, p, e, length)[0]
    parts = [ref.binomial(L, key, float(nc), p, c * length + e, length)[0] for c, nc in enumerate((512, 512, 276))]
    assert whole == sum(parts)
    whole = ref.poisson(L, key, 700.0, e, length)[0]
    parts = [ref.poisson(L, key, 700.0 / 3.0, c * length + e, length)[0] for c in range(3)]
    assert whole == sum(parts)


def test_edge_cases():
    L = lib()

    def s(fam, a, b=0.0, e=1):
        return ref.sample(L, fam, a, b, 5, 2, 9, 1, e, 4)[0]

    for fam, a, b in [("normal", 0.0, -1.0), ("normal", NAN, 1.0), ("normal", 0.0, INF), ("normal", INF, 1.0),
                      ("isonormal", 0.0, -0.5), ("bernoulli", -0.1, 0), ("bernoulli", 1.1, 0), ("bernoulli", NAN, 0),
                      ("exponential", 0.0, 0), ("exponential", -1.0, 0), ("exponential", INF, 0), ("exponential", NAN, 0),
                      ("uniform", 2.0, 1.0), ("uniform", NAN, 1.0), ("uniform", 0.0, INF),
                      ("binomial", 10.0, -0.1), ("binomial", 10.0, 1.5), ("binomial", 10.0, NAN), ("binomial", -1.0, 0.5),
                      ("binomial", 2.5, 0.5), ("binomial", 2.0 ** 21, 0.5), ("binomial", NAN, 0.5),
                      ("poisson", -1.0, 0), ("poisson", NAN, 0), ("poisson", INF, 0), ("poisson", 64 * 256.0 + 1.0, 0),
                      ("gamma", 0.0, 1.0), ("gamma", -2.0, 1.0), ("gamma", NAN, 1.0), ("gamma", INF, 1.0),
                      ("gamma", 1.0, 0.0), ("gamma", 1.0, NAN), ("invgamma", NAN, 1.0), ("invgamma", 1.0, -1.0),
                      ("beta", 0.0, 1.0), ("beta", 1.0, NAN), ("beta", INF, 1.0)]:
        assert math.isnan(s(fam, a, b)), (fam, a, b)
    for n in (0.0, 1.0, 81.0, 1300.0):
        assert s("binomial", n, 0.0) == 0.0 and s("binomial", n, 1.0) == n
        assert 0.0 <= s("binomial", n, 0.5) <= n
    assert s("bernoulli", 0.0) == 0.0 and s("bernoulli", 1.0) == 1.0
    assert s("poisson", 0.0) == 0.0 and s("normal", 1.5, 0.0) == 1.5 and s("uniform", 2.0, 2.0) == 2.0
    assert not math.isnan(s("poisson", 64 * 256.0))
    # a pure function of (seed, chain, iteration, node, element); elements 2q and 2q + 1 share a normal pair
    assert s("gamma", 0.4, 2.0) == s("gamma", 0.4, 2.0) and s("gamma", 0.4, 2.0, e=1) != s("gamma", 0.4, 2.0, e=2)
    assert ref.sample(L, "normal", 0, 1, 5, 2, 9 + 2 ** 32, 1, 1, 4) == ref.sample(L, "normal", 0, 1, 5, 2, 9, 1, 1, 4)
    # the edge flag: a uniform on a cdf step
    u = L.orc_uniform(5, 2, 9, ref.pb(1), ref.SUB_UNIFORM, 1)
    assert ref.sample(L, "bernoulli", u, 0, 5, 2, 9, 1, 1, 4) == (0.0, True)
    assert ref.sample(L, "bernoulli", u * (1 + 1e-6), 0, 5, 2, 9, 1, 1, 4) == (1.0, False)


# ---------------------------------------------------------------- the models of the GPU tests
LINE_START, LINE_THIN, SEED = 3, 2, 7


def _sqrt(x):
    """IEEE sqrt: NaN below zero."""
    return math.sqrt(x) if x >= 0 else NAN


def line_pdesc(y_id):
    d = mref.line_desc()
    return {"cols": d["cols"], "nodes": {"y": {
        "id": y_id, "fam": "isonormal", "len": 5,
        "params": lambda v: (v["beta"][0] + v["beta"][1] * mref.LINE_X, _sqrt(v["s2"][0]))}}}


def line_pdraws():
    """5 x 3 x 70, with three draws outside the domain."""
    v = line_draws(5, 70)
    v[1, 2, 13] = -0.5       # s2 < 0
    v[2, 0, 69] = NAN        # beta[1]
    v[4, 1, 0] = INF         # beta[2]
    return v


def seeds_pdesc(data, r_id):
    d = mref.seeds_desc(data)
    n = np.asarray(data["n"], float)
    x1, x2 = np.asarray(data["x1"], float), np.asarray(data["x2"], float)

    def params(v):
        eta = v["alpha0"][0] + v["alpha1"][0] * x1 + v["alpha2"][0] * x2 + v["alpha12"][0] * x1 * x2 + v["b"]
        return n, mref.invlogit(eta)

    return {"cols": d["cols"], "nodes": {"r": {"id": r_id, "fam": "binomial", "len": 21, "params": params}}}


def rats_pdesc(y, rat, Xm, y_id):
    d = mref.rats_desc(y, rat, Xm)
    rat, Xm = np.asarray(rat, int), np.asarray(Xm, float)
    return {"cols": d["cols"], "nodes": {"y": {
        "id": y_id, "fam": "isonormal", "len": 150,
        "params": lambda v: (v["alpha"][rat] + v["beta"][rat] * Xm, math.sqrt(v["s2_c"][0]))}}}


# A synthetic model whose observed nodes cover every family; th (4 sampled values) carries the parameters
# through single IEEE operations, so the restatement's parameters have the device's bits.
AF_XS = np.array([-1.0, 0.5, 2.0, 3.5, 0.25])
AF_W = np.array([1.0, 0.5, 0.25, 1.0, 0.75, 0.125])
AF_NB = np.array([81.0, 1300.0, 512.0, 513.0, 1.0, 7.0])     # 1300 = 512 + 512 + 276
AF_LAM = np.array([3.0, 700.0, 0.5, 256.0])                  # th[3] in [0.8, 1.05]: 700 th[3] is three pieces
AF_SH = np.array([0.4, 3.5, 1.0])                            # shapes below and above 1
AF_KEYS = ["yn", "ym", "yb", "ye", "yu", "ybi", "yp", "yg", "yig", "ybe", "ys"]


def allfam_model(mamba):
    ir = mamba.ir
    m = ir.Model(
        th=ir.Stochastic(1, lambda: ir.Normal(0, 10)),
        yn=ir.Stochastic(1, lambda th, xs: ir.Normal(th[1] + th[2] * xs, th[3]), False),
        ym=ir.Stochastic(1, lambda th, xs: ir.MvNormal(th[1] * xs, ir.sqrt(th[3])), False),
        yb=ir.Stochastic(1, lambda th, w: ir.Bernoulli(th[4] * w), False),
        ye=ir.Stochastic(1, lambda th, w: ir.Exponential(th[3] * w), False),
        yu=ir.Stochastic(1, lambda: ir.Uniform(-1.0, 3.0), False),
        ybi=ir.Stochastic(1, lambda nb, th, w: ir.Binomial(nb, th[4] * w), False),
        yp=ir.Stochastic(1, lambda th, lam: ir.Poisson(th[3] * lam), False),
        yg=ir.Stochastic(1, lambda th, sh: ir.Gamma(th[3] * sh, th[2] + 3.0), False),
        yig=ir.Stochastic(1, lambda th, sh: ir.InverseGamma(th[3] + sh, th[3]), False),
        ybe=ir.Stochastic(1, lambda th, sh: ir.Beta(th[3] * sh, th[4] + sh), False),
        ys=ir.Stochastic(lambda th: ir.Normal(th[1], th[3]), False))
    m.setinputs({"xs": AF_XS, "w": AF_W, "nb": AF_NB, "lam": AF_LAM, "sh": AF_SH})
    m.setsamplers([mamba.AMWG(["th"], 1.0)])
    return m


def allfam_inits(K):
    obs = {"yn": np.zeros(5), "ym": np.zeros(5), "yb": np.array([0.0, 1, 0, 1, 1, 0]), "ye": np.ones(6),
           "yu": np.ones(6), "ybi": np.array([20.0, 600, 100, 100, 1, 3]), "yp": np.array([2.0, 690, 0, 250]),
           "yg": np.ones(3), "yig": np.ones(3), "ybe": np.full(3, 0.5), "ys": 0.25}
    return [{**obs, "th": [0.1, 0.2, 1.0, 0.5]} for _ in range(K)]


def allfam_pdesc(ids):
    def th(v, k):
        return v["th"][k - 1]

    nodes = {
        "yn": ("normal", 5, lambda v: (th(v, 1) + th(v, 2) * AF_XS, th(v, 3))),
        "ym": ("isonormal", 5, lambda v: (th(v, 1) * AF_XS, _sqrt(th(v, 3)))),
        "yb": ("bernoulli", 6, lambda v: (th(v, 4) * AF_W, 0.0)),
        "ye": ("exponential", 6, lambda v: (th(v, 3) * AF_W, 0.0)),
        "yu": ("uniform", 6, lambda v: (-1.0, 3.0)),
        "ybi": ("binomial", 6, lambda v: (AF_NB, th(v, 4) * AF_W)),
        "yp": ("poisson", 4, lambda v: (th(v, 3) * AF_LAM, 0.0)),
        "yg": ("gamma", 3, lambda v: (th(v, 3) * AF_SH, th(v, 2) + 3.0)),
        "yig": ("invgamma", 3, lambda v: (th(v, 3) + AF_SH, th(v, 3))),
        "ybe": ("beta", 3, lambda v: (th(v, 3) * AF_SH, th(v, 4) + AF_SH)),
        "ys": ("normal", 1, lambda v: (th(v, 1), th(v, 3))),
    }
    return {"cols": {"th": [0, 1, 2, 3]},
            "nodes": {k: {"id": ids[k], "fam": f, "len": ln, "params": p, "scalar": k == "ys"}
                      for k, (f, ln, p) in nodes.items()}}


def allfam_draws(n=3, K=37, seed=21):
    """th[1], th[2] free, th[3] in [0.8, 1.05], th[4] in (0.3, 0.95); four draws outside the domains."""
    rng = np.random.default_rng(seed)
    v = np.empty((n, 4, K))
    v[:, 0, :] = rng.normal(0.5, 1.0, (n, K))
    v[:, 1, :] = rng.normal(-0.2, 0.4, (n, K))
    v[:, 2, :] = rng.uniform(0.8, 1.05, (n, K))
    v[:, 3, :] = rng.uniform(0.3, 0.95, (n, K))
    v[0, 2, 5] = -1.0        # sigma, scale, lambda, shape < 0
    v[1, 3, 36] = 1.7        # p > 1
    v[2, 2, 0] = NAN
    v[2, 0, 20] = INF
    return v


def bigvec_short(mamba, m, mz, z):
    """tests/test_gpu_modelstats.py's model (theta[1..m], tau; nvalues = m + 1) with the observed z cut to its
    first mz elements, so that the state images and a result tile of mz columns share the 64 KiB of LDS:
    m = 300, mz = 150: (301 + 151) doubles per chain, 16 chains fit, 32 do not;
    m = 500, mz = 400: (501 + 401) doubles per chain, 8 chains fit, 16 do not."""
    from test_gpu_modelstats import bigvec
    M = bigvec(mamba, m, z)
    M.nodes[0].len = mz
    return M


def bigvec_pdesc(z, m, mz):
    return {"cols": {"theta": list(range(m))},
            "nodes": {"z": {"id": 0, "fam": "normal", "len": mz, "params": lambda v: (v["theta"][:mz], 0.5)}}}


def bigvec_draws(m, n=2, K=9):
    rng = np.random.default_rng(m)
    z = rng.normal(0.0, 2.0, m)
    v = np.empty((n, m + 1, K))
    v[:, :m, :] = z[None, :, None] + rng.normal(0.0, 0.5, (n, m, K))
    v[:, m, :] = rng.normal(0.0, 1.0, (n, K))
    return z, v


def _ir_model(mamba, name, K=2):
    from test_gpu_modelstats import ir_line, ir_rats, ir_seeds
    return {"line": ir_line, "seeds": ir_seeds, "rats": ir_rats}[name](mamba, K)[0]


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(draws, description, keys, expected n x P x K, edge draws) of a GPU test's fixture, computed once.
    Row i has iteration LINE_START + i * LINE_THIN, seed SEED, chain_offset 0."""
    import _mamba_path
    mamba = _mamba_path.load()
    if name == "line":
        v, d, keys = line_pdraws(), line_pdesc(mamba.abi.MMB_LINE_Y), ["y"]
    elif name == "ir_line":
        m = _ir_model(mamba, "line")
        v, d, keys = line_pdraws(), line_pdesc(m.stats_table()["ids"]["y"]), ["y"]
    elif name == "seeds":
        from test_gpu_modelstats import seeds_draws
        m = _ir_model(mamba, "seeds")
        v, d, keys = seeds_draws(), seeds_pdesc(mamba.ir.SEEDS, m.stats_table()["ids"]["r"]), ["r"]
    elif name == "rats":
        from test_gpu_modelstats import rats_draws
        m = _ir_model(mamba, "rats")
        inp = mamba.ir.rats_inputs()
        v = rats_draws(mamba)
        d, keys = rats_pdesc(inp["y"], np.asarray(inp["rat"], int) - 1, inp["Xm"], m.stats_table()["ids"]["y"]), ["y"]
    elif name == "allfam":
        m = allfam_model(mamba)
        m.init_matrix(allfam_inits(1), 1)
        v, d, keys = allfam_draws(), allfam_pdesc(m.stats_table()["ids"]), list(AF_KEYS)
    elif name in ("big300", "big500"):
        m, mz = (300, 150) if name == "big300" else (500, 400)
        z, v = bigvec_draws(m)
        d, keys = bigvec_pdesc(z, m, mz), ["z"]
    else:
        raise KeyError(name)
    want, edges = ref.predict_draws(lib(), v, d, keys, SEED, 0, LINE_START, LINE_THIN)
    want.setflags(write=False)
    return v, d, keys, want, edges


FIXTURES = ["line", "ir_line", "seeds", "rats", "allfam", "big300", "big500"]


@pytest.mark.parametrize("name", FIXTURES)
def test_gpu_fixtures_have_no_edge_draw(name):
    """The condition that lets the GPU tests demand exact equality of the discrete families."""
    v, d, keys, want, edges = fixture(name)
    assert edges == 0
    assert want.shape == (v.shape[0], sum(ref.widths(d, keys)), v.shape[2])
    if name == "allfam":   # the fixture reaches what it is meant to reach
        j = dict(zip(keys, np.cumsum([0] + ref.widths(d, keys))))
        assert np.isnan(want[0, :, 5]).sum() > 20 and np.isnan(want[1, j["ybi"], 36]) and np.isnan(want[2, j["yn"], 20])
        assert not np.isnan(want[0, j["yu"]:j["yu"] + 6, 5]).any()          # Uniform reads no draw
        ok = np.isfinite(want)
        assert ok.mean() > 0.95 and want[:, j["ybi"] + 1, :][ok[:, j["ybi"] + 1, :]].max() <= 1300
    if name == "line":
        assert np.isnan(want[1, :, 13]).all() and np.isnan(want[2, :, 69]).all() and np.isnan(want[4, :, 0]).all()
        assert np.isfinite(want).sum() == want.size - 15


# ---------------------------------------------------------------- host logic against an engine-shaped fake
def _line_fake(mamba, value, **kw):
    ids = mamba.line().stats_table()["ids"]
    return ref.FakeEngine(lib(), value, line_pdesc(ids["y"]), {v: k for k, v in ids.items()}, **kw)


def _line_sim(mamba, v, eng, start=LINE_START, thin=LINE_THIN):
    m = mamba.line()
    m.setinputs(mamba.model.LINE_DATA)
    return mamba.Chains(v, m.monitor_names, start, thin, np.arange(1, v.shape[2] + 1), m, eng)


def test_predict_names_keys_and_window(mamba):
    v = line_pdraws()[:, :, :6]
    eng = _line_fake(mamba, v, seed=SEED)
    sim = _line_sim(mamba, v, eng)
    pp = sim.predict()
    assert pp.names == ["y[1]", "y[2]", "y[3]", "y[4]", "y[5]"] and pp.value.shape == (5, 5, 6)
    assert pp.start == LINE_START and pp.thin == LINE_THIN and np.array_equal(pp.chains, sim.chains)
    assert pp.model is sim.model and pp.range == sim.range
    assert eng.calls[-1] == ([mamba.abi.MMB_LINE_Y], SEED, LINE_START, LINE_THIN, 0, 5)   # the chains' own seed
    want = fixture("line")[3][:, :, :6]
    assert np.array_equal(pp.value, want, equal_nan=True)
    assert np.array_equal(mamba.predict(sim, "y").value, want, equal_nan=True)            # one name
    w = sim.predict(["y"], rows=(2, 5))
    assert w.start == LINE_START + 2 * LINE_THIN and w.thin == LINE_THIN and list(w.range) == list(sim.range)[2:5]
    assert eng.calls[-1][2:] == (LINE_START, LINE_THIN, 2, 5)                             # the full call's iterations
    assert np.array_equal(w.value, want[2:5], equal_nan=True)
    assert not np.array_equal(sim.predict(seed=SEED + 1).value, want, equal_nan=True)
    assert eng.calls[-1][1] == SEED + 1
    # names of the node-IR models: vector nodes by element, a scalar node by its bare name
    m = allfam_model(mamba)
    m.init_matrix(allfam_inits(1), 1)
    assert m.keys("output") == AF_KEYS
    nm = mamba.modelstats.predict_names(m, ["ys", "yg", "yn"])
    assert nm == ["ys", "yg[1]", "yg[2]", "yg[3]"] + [f"yn[{i}]" for i in range(1, 6)]
    assert nm == ref.names(allfam_pdesc(m.stats_table()["ids"]), ["ys", "yg", "yn"])


def test_predict_argument_errors(mamba):
    v = line_pdraws()[:, :, :3]
    sim = _line_sim(mamba, v, _line_fake(mamba, v))
    msg = "nodekeys are not all observed Stochastic nodess : y"       # modelstats.jl:78-82, verbatim
    for keys in ("beta", ["y", "s2"], ["nu"]):
        with pytest.raises(mamba.ArgumentError, match=msg):
            sim.predict(keys)
        with pytest.raises(mamba.ArgumentError, match=msg):
            sim.predict_summary(keys)
    for rows in ((0, 0), (3, 2), (-1, 2), (0, 6)):
        with pytest.raises(mamba.ArgumentError, match="kept draws"):
            sim.predict(rows=rows)
    with pytest.raises(mamba.ArgumentError):
        sim.predict([])
    with pytest.raises(mamba.ArgumentError):
        _line_sim(mamba, v, None).predict()                      # no device-kept draws
    with pytest.raises(mamba.ArgumentError):
        mamba.Chains(v, ["beta[1]", "beta[2]", "s2"], 1, 1, [1, 2, 3], None, None).predict()
    with pytest.raises(mamba.ArgumentError, match="alpha"):      # hand-lowered rats: alpha, beta are not monitored
        mamba.predict_sharded(_line_fake(mamba, v), mamba.rats())
    from test_modelstats import _ir
    with pytest.raises(mamba.ArgumentError, match="b is not monitored"):
        mamba.predict_sharded(_line_fake(mamba, v), _ir(mamba, "seeds"), ["r"])


def test_predict_moments_sharded(mamba):
    from test_modelstats import _SumOverRanks
    import threading
    v = line_draws(6, 8)
    m = mamba.line()
    m.setinputs(mamba.model.LINE_DATA)
    one = mamba.predict_moments_sharded(_line_fake(mamba, v, seed=SEED), m, None, None, None, LINE_START, LINE_THIN)
    yhat = ref.predict_draws(lib(), v, line_pdesc(2), ["y"], SEED, 0, LINE_START, LINE_THIN)[0]
    pooled = yhat.transpose(1, 0, 2).reshape(5, -1)
    np.testing.assert_allclose(one[:, 0], pooled.mean(1), rtol=1e-12)
    np.testing.assert_allclose(one[:, 1], pooled.std(1, ddof=1), rtol=1e-12)
    red = _SumOverRanks(2)
    out = [None, None]

    def rank(r, part, off):
        eng = _line_fake(mamba, part, seed=SEED, chain_offset=off)
        out[r] = mamba.predict_moments_sharded(eng, m, ["y"], red, None, LINE_START, LINE_THIN)

    ts = [threading.Thread(target=rank, args=(r, part, off), daemon=True)
          for r, (part, off) in enumerate(((v[:, :, :3], 0), (v[:, :, 3:], 3)))]
    for t in ts:
        t.start()
    for t in ts:
        t.join(60)
    assert out[0] is not None and out[1] is not None
    np.testing.assert_allclose(out[0], one, rtol=1e-12)
    np.testing.assert_allclose(out[1], one, rtol=1e-12)
