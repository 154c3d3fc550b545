"""Model statistics on the device (modelstats.hip through mmb_draws_logpdf / mmb_draws_deviance /
mmb_logpdf_at, mamba.jl_amd/modelstats.py) against the restatement tests/modelstats_ref.py.

Tolerances.  Per-draw log densities: rtol 1e-12 + atol 1e-9, the project's bound for a block log
density against scipy (tests/test_oracle.py:39,54); the restatement sums elements with math.fsum,
the device in lane partials and a butterfly, at most 150 terms; -Inf must be exactly -Inf.  The
four DIC figures: rtol 1e-8, the project's bound for derived figures (no cancellation in the
variance for these inputs: tests/test_modelstats.py asserts S2 / (S2 - S1^2 / N) < 2 on the line
input).  mmb_logpdf_at against mmb_draws_logpdf: bit for bit.  Draws are uploaded with set_draws."""
import ctypes as C
import math
import threading

import numpy as np
import pytest

import modelstats_ref as ref
from test_modelstats import _SumOverRanks, line_draws

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-12, 1e-9


def close(got, want):
    got, want = np.asarray(got), np.asarray(want)
    inf = np.isneginf(want)
    assert np.array_equal(np.isneginf(got), inf)
    np.testing.assert_allclose(got[~inf], want[~inf], rtol=RTOL, atol=ATOL)


# ---------------------------------------------------------------- engines
def line_engine(mamba, K):
    m = mamba.line()
    m.setinputs(mamba.model.LINE_DATA)
    m.setsamplers([mamba.AMWG(["beta", "s2"], 1.0)])
    eng = mamba.Engine(m)
    eng.init_chains(mamba.model.line_init_matrix(K, seed=3), seed=7)
    return m, eng


def ir_line(mamba, K):
    ir = mamba.ir
    m = ir.line_model().setinputs(mamba.model.LINE_DATA)
    m.setsamplers([mamba.AMWG(["beta", "s2"], 1.0)])
    v = mamba.model.line_init_matrix(K, seed=3)
    V = m.init_matrix([{"y": [1.0, 3, 3, 3, 5], "beta": v[k, :2], "s2": v[k, 2]} for k in range(K)], K)
    return m, V


def ir_seeds(mamba, K):
    """doc/examples/seeds.jl:16-56 with the random effects b monitored."""
    ir = mamba.ir
    m = ir.Model(
        r=ir.Stochastic(1, lambda alpha0, alpha1, x1, alpha2, x2, alpha12, b, n:
                        ir.Binomial(n, ir.invlogit(alpha0 + alpha1 * x1 + alpha2 * x2 + alpha12 * x1 * x2 + b)), False),
        b=ir.Stochastic(1, lambda s2: ir.Normal(0, ir.sqrt(s2))),
        alpha0=ir.Stochastic(lambda: ir.Normal(0, 1000)),
        alpha1=ir.Stochastic(lambda: ir.Normal(0, 1000)),
        alpha2=ir.Stochastic(lambda: ir.Normal(0, 1000)),
        alpha12=ir.Stochastic(lambda: ir.Normal(0, 1000)),
        s2=ir.Stochastic(lambda: ir.InverseGamma(0.001, 0.001)))
    m.setinputs(ir.SEEDS)
    m.setsamplers([mamba.AMM(["alpha0", "alpha1", "alpha2", "alpha12"], 0.01 * np.eye(4)), mamba.AMWG("b", 0.01),
                   mamba.AMWG("s2", 0.1)])
    return m, m.init_matrix([ir.seeds_inits()[k % 2] for k in range(K)], K)


def ir_rats(mamba, K):
    """doc/examples/rats.jl:48-97 with every sampled node (and the Logical alpha0) monitored."""
    ir = mamba.ir
    m = ir.Model(
        y=ir.Stochastic(1, lambda alpha, beta, rat, Xm, s2_c:
                        ir.MvNormal(alpha[rat] + beta[rat] * Xm, ir.sqrt(s2_c)), False),
        alpha=ir.Stochastic(1, lambda mu_alpha, s2_alpha: ir.Normal(mu_alpha, ir.sqrt(s2_alpha))),
        alpha0=ir.Logical(lambda mu_alpha, xbar, mu_beta: mu_alpha - xbar * mu_beta),
        mu_alpha=ir.Stochastic(lambda: ir.Normal(0.0, 1000)),
        s2_alpha=ir.Stochastic(lambda: ir.InverseGamma(0.001, 0.001)),
        beta=ir.Stochastic(1, lambda mu_beta, s2_beta: ir.Normal(mu_beta, ir.sqrt(s2_beta))),
        mu_beta=ir.Stochastic(lambda: ir.Normal(0.0, 1000)),
        s2_beta=ir.Stochastic(lambda: ir.InverseGamma(0.001, 0.001)),
        s2_c=ir.Stochastic(lambda: ir.InverseGamma(0.001, 0.001)))
    m.setinputs(ir.rats_inputs())
    m.setsamplers(mamba.model.rats_scheme_reference())
    return m, m.init_matrix(ir.rats_inits_ls(K, seed=2), K)


def ir_engine(mamba, monkeypatch, m, V, jit=False):
    if not jit:
        monkeypatch.setenv("MMB_IR_JIT", "0")
    eng = mamba.Engine(m)
    assert eng.ir_jit()[0] == jit, eng.ir_jit()
    eng.init_chains(V, seed=7)
    return eng


def ids_of(mamba, m, keys):
    return mamba.modelstats.node_ids(m, keys)


# ---------------------------------------------------------------- draws
def seeds_draws(n=5, K=70, seed=8):
    rng = np.random.default_rng(seed)
    v = np.empty((n, 26, K))
    v[:, :21, :] = rng.normal(0.0, 0.3, (n, 21, K))
    for j, mu in enumerate((-0.55, 0.08, 1.35, -0.82)):          # the published posterior means (seeds.rst)
        v[:, 21 + j, :] = mu + rng.normal(0.0, 0.05, (n, K))
    v[:, 25, :] = 0.09 * np.exp(rng.normal(0.0, 0.1, (n, K)))
    return v


def rats_draws(mamba, n=3, K=33, seed=9):
    """rats_init_ls rows plus jitter, in the monitored-column order of ir_rats; the alpha0 column holds a
    value the Logical could never take: it must not be read."""
    rng = np.random.default_rng(seed)
    c = mamba.model.rats_init_ls(n * K, seed=4).reshape(n, K, 65)   # [s2_c, alpha, mu_alpha, s2_alpha, beta, ...]
    v = np.empty((n, 66, K))
    v[:, 0:30, :] = (c[:, :, 1:31] + rng.normal(0.0, 0.5, (n, K, 30))).transpose(0, 2, 1)
    v[:, 30, :] = 1e300
    v[:, 31, :] = c[:, :, 31] + rng.normal(0.0, 0.1, (n, K))
    v[:, 32, :] = c[:, :, 32] * np.exp(rng.normal(0.0, 0.05, (n, K)))
    v[:, 33:63, :] = (c[:, :, 33:63] + rng.normal(0.0, 0.05, (n, K, 30))).transpose(0, 2, 1)
    v[:, 63, :] = c[:, :, 63] + rng.normal(0.0, 0.1, (n, K))
    v[:, 64, :] = c[:, :, 64] * np.exp(rng.normal(0.0, 0.05, (n, K)))
    v[:, 65, :] = c[:, :, 0] * np.exp(rng.normal(0.0, 0.05, (n, K)))
    return v


def rats_desc(mamba):
    inp = mamba.ir.rats_inputs()
    return ref.rats_desc(inp["y"], np.asarray(inp["rat"], int) - 1, inp["Xm"])


@pytest.fixture(scope="module")
def line_ref():
    v = line_draws()
    d = ref.line_desc()
    return v, {tuple(k): ref.logpdf_draws(v, d, k) for k in (["y"], ["beta", "s2", "y"], ["s2"])}


# ---------------------------------------------------------------- cases
def test_line_hand_lowered(mamba, line_ref):
    v, want = line_ref
    m, eng = line_engine(mamba, v.shape[2])
    eng.set_draws(v)
    for keys, w in want.items():
        got = eng.draws_logpdf(ids_of(mamba, m, list(keys)))
        assert got.shape == (37, 70)
        close(got, w)
    sim = mamba.Chains(v, m.monitor_names, 201, 2, np.arange(1, 71), m, eng)
    lp = sim.logpdf("y")
    assert lp.value.shape == (37, 1, 70) and lp.names == ["logpdf"]
    assert lp.range == sim.range and np.array_equal(lp.chains, sim.chains)
    close(lp.value[:, 0, :], want[("y",)])
    close(mamba.logpdf(sim).value[:, 0, :], ref.logpdf_draws(v, ref.line_desc(), ["y", "beta", "s2"]))
    v2 = v.copy()
    v2[5, 2, 13] = -1.0                       # outside the support of s2 at one (row, chain)
    eng.set_draws(v2)
    got = eng.draws_logpdf(ids_of(mamba, m, ["s2"]))
    w = want[("s2",)].copy()
    w[5, 13] = -math.inf
    assert got[5, 13] == -math.inf
    close(got, w)


def test_ir_line_equals_hand_lowered(mamba, monkeypatch, line_ref):
    v, want = line_ref
    m, V = ir_line(mamba, v.shape[2])
    eng = ir_engine(mamba, monkeypatch, m, V)
    eng.set_draws(v)
    for keys, w in want.items():
        close(eng.draws_logpdf(ids_of(mamba, m, list(keys))), w)


def test_ir_seeds(mamba, monkeypatch):
    v = seeds_draws()
    m, V = ir_seeds(mamba, v.shape[2])
    assert m.monitor_names[:2] == ["b[1]", "b[2]"] and m.monitor_names[21:] == ["alpha0", "alpha1", "alpha2",
                                                                                 "alpha12", "s2"]
    eng = ir_engine(mamba, monkeypatch, m, V)
    eng.set_draws(v)
    d = ref.seeds_desc(mamba.ir.SEEDS)
    for keys in (["r"], ["b", "s2"], m.keys("stochastic")):
        close(eng.draws_logpdf(ids_of(mamba, m, keys)), ref.logpdf_draws(v, d, keys))
    sim = mamba.Chains(v, m.monitor_names, 1, 1, np.arange(1, v.shape[2] + 1), m, eng)
    got, rows, cols = sim.dic()
    np.testing.assert_allclose(got, ref.dic(v, d, ["r"])[0], rtol=1e-8)


def test_ir_rats(mamba, monkeypatch):
    v = rats_draws(mamba)
    m, V = ir_rats(mamba, v.shape[2])
    assert len(m.monitor_names) == 66 and m.monitor_names[30] == "alpha0" and m.nvalues == 65
    eng = ir_engine(mamba, monkeypatch, m, V)
    eng.set_draws(v)
    d = rats_desc(mamba)
    for keys in (["y"], ["alpha", "beta"], m.keys("stochastic")):
        close(eng.draws_logpdf(ids_of(mamba, m, keys)), ref.logpdf_draws(v, d, keys))


class _BigVec:
    """A node-IR model written at the C ABI: theta[1..m] ~ Normal(0, 2) (sampled values, in no block),
    tau ~ Normal(0, 1) in an AMWG block, z[1..m] ~ Normal(theta, 0.5) observed; theta and tau monitored.
    nvalues = m + 1: larger than a model lowered from ir.py can have (8 blocks of at most 32 elements)."""
    input_names = []

    def __init__(self, mamba, m, z):
        a = mamba.abi
        self.kind = a.MMB_MODEL_IR
        self.m = m
        op = a.IR_OP
        # code: [0] vali 0, end; [2] const 0 (0.5), end; [4] const 1 (0.0), end; [6] const 2 (2.0), end;
        #       [8] const 3 (1.0), end
        self.code = np.array([op["vali"] << 24 | 0, 0, op["const"] << 24 | 0, 0, op["const"] << 24 | 1, 0,
                              op["const"] << 24 | 2, 0, op["const"] << 24 | 3, 0], dtype=np.int32)
        self.consts = np.array([0.5, 0.0, 2.0, 1.0])
        self.pool = np.concatenate([np.asarray(z, float), [0.0]])
        self.nodes = (a.IrNode * 3)()
        for N, (fam, fixed, off, ln, e0, e1) in zip(self.nodes, [(a.MMB_IR_NORMAL, 1, 0, m, 0, 2),
                                                                  (a.MMB_IR_NORMAL, 0, 0, m, 4, 6),
                                                                  (a.MMB_IR_NORMAL, 0, m, 1, 4, 8)]):
            N.family, N.fixed, N.off, N.len, N.cterm = fam, fixed, off, ln, -1
            N.expr[0], N.expr[1], N.expr[2] = e0, e1, -1
        self.mon = np.array([1, 2], dtype=np.int32)
        self.samplers = [mamba.AMWG("tau", 1.0)]

    def spec(self):
        return self._spec

    def ir(self):
        return self._ir

    def data_arrays(self):
        return []


def bigvec(mamba, m, z):
    a = mamba.abi
    M = _BigVec(mamba, m, z)
    sp = a.ModelSpec()
    sp.model, sp.nblocks = a.MMB_MODEL_IR, 1
    b = sp.blocks[0]
    b.sampler, b.nnodes, b.adapt, b.transform, b.batchsize, b.target, b.dim = a.MMB_SAMPLER_AMWG, 1, 0, 1, 50, 0.44, 1
    b.nodes[0] = 2
    M.tuning = np.array([1.0])
    b.ntuning, b.tuning = 1, a.dptr(M.tuning)
    irm = a.IrModel()
    irm.nvalues, irm.nnodes, irm.nodes = m + 1, 3, M.nodes
    irm.ncode, irm.code = M.code.size, M.code.ctypes.data_as(C.POINTER(C.c_int32))
    irm.nconst, irm.consts = M.consts.size, a.dptr(M.consts)
    irm.npool, irm.pool = m, a.dptr(M.pool)
    irm.nmon, irm.mon = 2, M.mon.ctypes.data_as(C.POINTER(C.c_int32))
    irm.stack = 2
    irm.blocks[0].nterms = 1
    irm.blocks[0].term[0] = 2
    irm.blocks[0].trans[0] = 1
    M._spec, M._ir = sp, irm
    return M


@pytest.mark.parametrize("m", [300, 500])      # tiles of 16 and of 8 chains (modelstats.hip: 64 KiB of LDS)
def test_large_state_tiles(mamba, monkeypatch, m):
    n, K = 2, 9
    rng = np.random.default_rng(m)
    z = rng.normal(0.0, 2.0, m)
    v = np.empty((n, m + 1, K))
    v[:, :m, :] = z[None, :, None] + rng.normal(0.0, 0.5, (n, m, K))
    v[:, m, :] = rng.normal(0.0, 1.0, (n, K))
    M = bigvec(mamba, m, z)
    monkeypatch.setenv("MMB_IR_JIT", "0")
    eng = mamba.Engine(M)
    assert eng.P == m + 1 and eng.pmon == m + 1
    eng.init_chains(np.zeros((K, m + 1)), seed=1)
    eng.set_draws(v)
    d = ref.bigvec_desc(z, m)
    close(eng.draws_logpdf([0]), ref.logpdf_draws(v, d, ["z"]))
    close(eng.draws_logpdf([1, 0]), ref.logpdf_draws(v, d, ["theta", "z"]))
    assert eng.logpdf_at([0, 1], v[1, :, 8]) == eng.draws_logpdf([0, 1])[1, 8]


def test_logpdf_at_and_deviance(mamba, monkeypatch):
    v = line_draws()
    m, eng = line_engine(mamba, v.shape[2])
    eng.set_draws(v)
    vr = rats_draws(mamba)
    mr, V = ir_rats(mamba, vr.shape[2])
    er = ir_engine(mamba, monkeypatch, mr, V)
    er.set_draws(vr)
    for e, mm, val, keys in ((eng, m, v, ["beta", "s2", "y"]), (er, mr, vr, mr.keys("stochastic"))):
        ids = ids_of(mamba, mm, keys)
        lp = e.draws_logpdf(ids)
        n, _, K = val.shape
        for i, k in [(0, 0), (n - 1, K - 1), (1, 31), (2, 32)]:
            assert e.logpdf_at(ids, val[i, :, k]) == lp[i, k]       # bit for bit: one code path
        shift = float((-2.0 * lp).min()) - 1.0      # every D - shift >= 1: sums without cancellation
        got = e.draws_deviance(ids, shift)
        D = -2.0 * lp - shift
        want = np.array([[math.fsum(D[:, k]), math.fsum(D[:, k] ** 2)] for k in range(K)])
        np.testing.assert_allclose(got, want, rtol=1e-12)


def _line_sim(mamba, K, off=0, allK=256):
    m = mamba.line()
    m.setsamplers([mamba.AMWG(["beta", "s2"], 1.0)])
    init = mamba.model.line_init_matrix(allK, seed=5)[off:off + K]
    return mamba.mcmc(m, mamba.model.LINE_DATA, init, 400, burnin=200, chains=K, chain_offset=off, seed=11,
                      keep_device=True)


def test_dic_on_sampler_output(mamba):
    sim = _line_sim(mamba, 256)
    assert sim.value.shape == (200, 3, 256)
    got, rows, cols = sim.dic()
    assert rows == ["pD", "pV"] and cols == ["DIC", "Effective Parameters"]
    want, _ = ref.dic(sim.value, ref.line_desc(), ["y"])
    np.testing.assert_allclose(got, want, rtol=1e-8)
    assert np.array_equal(mamba.dic(sim)[0], got)
    # two engines over the chain halves (global chain ids key the streams: the same draws)
    parts = [_line_sim(mamba, 128, 0), _line_sim(mamba, 128, 128)]
    assert np.array_equal(np.concatenate([p.value for p in parts], axis=2), sim.value)
    red = _SumOverRanks(2)
    out = [None, None]

    def rank(r):
        out[r] = mamba.dic_sharded(parts[r].engine, parts[r].model, allreduce_sum=red)[0]

    ts = [threading.Thread(target=rank, args=(r,), daemon=True) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert out[0] is not None and out[1] is not None
    np.testing.assert_allclose(out[0], got, rtol=1e-12)
    np.testing.assert_allclose(out[1], got, rtol=1e-12)


def test_nothing_is_disturbed(mamba):
    def fresh():
        m, eng = line_engine(mamba, 96)
        d = eng.run(60, burnin=20, thin=2, keep_device=True)
        return m, eng, d

    m, eng, d = fresh()
    _, twin, d2 = fresh()
    assert np.array_equal(d, d2)
    before = (eng.values(), eng.tune(), eng.draws(), eng.iter, eng.chain_order())
    sim = mamba.Chains(d, m.monitor_names, 22, 2, np.arange(1, 97), m, eng)
    sim.logpdf()
    sim.dic()
    eng.logpdf_at([2], d[0, :, 0])
    after = (eng.values(), eng.tune(), eng.draws(), eng.iter, eng.chain_order())
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert np.array_equal(eng.run(40, burnin=20, thin=2), twin.run(40, burnin=20, thin=2))
    assert np.array_equal(eng.values(), twin.values()) and np.array_equal(eng.tune(), twin.tune())


def test_errors(mamba, monkeypatch):
    ir = mamba.ir
    m = ir.rats_model().setinputs(ir.rats_inputs())
    m.setsamplers(mamba.model.rats_scheme_reference())
    V = m.init_matrix(ir.rats_inits_ls(4, seed=2), 4)
    eng = ir_engine(mamba, monkeypatch, m, V)
    eng.set_draws(np.ones((2, 3, 4)))
    sim = mamba.Chains(np.ones((2, 3, 4)), m.monitor_names, 1, 1, np.arange(1, 5), m, eng)
    with pytest.raises(mamba.ArgumentError, match="alpha"):
        sim.logpdf("y")
    y_id = m.stats_table()["ids"]["y"]
    with pytest.raises(RuntimeError, match="not monitored"):          # the engine's own refusal ...
        eng.draws_logpdf([y_id])
    with pytest.raises(mamba.ArgumentError, match="node alpha is not monitored"):   # ... and its mapping
        mamba.modelstats._engine_call(m, eng.draws_logpdf, [y_id])
    with pytest.raises(RuntimeError, match="invalid argument"):
        eng.draws_logpdf([list(m.order).index("alpha0")])             # a Logical
    with pytest.raises(RuntimeError, match="invalid argument"):
        eng.draws_deviance([len(m.order)], 0.0)                       # out of range
    with pytest.raises(RuntimeError, match="invalid argument"):
        eng.draws_logpdf([])
    # mu_beta and s2_c are monitored and read no unmonitored node
    ids = ids_of(mamba, m, ["mu_beta", "s2_c"])
    want = ref.normal_lp(1.0, 0.0, 1000.0) + ref.invgamma_lp(1.0, 0.001, 0.001)
    np.testing.assert_allclose(eng.draws_logpdf(ids), np.full((2, 4), want), rtol=RTOL, atol=ATOL)

    r = mamba.rats()
    r.setinputs(mamba.model.RATS_DATA)
    r.setsamplers(mamba.model.rats_scheme_gibbs_amm())
    with pytest.raises(RuntimeError, match="unsupported"):
        mamba.Engine(r).draws_logpdf([0])
    data, _ = mamba.model.logistic_data(64, 4)
    lg = mamba.logistic(64, 4)
    lg.setinputs(data)
    lg.setsamplers([mamba.NUTS("beta")])
    el = mamba.Engine(lg)
    with pytest.raises(RuntimeError, match="unsupported"):
        el.logpdf_at([0], np.zeros(4))

    ml, e0 = line_engine(mamba, 8)
    with pytest.raises(RuntimeError, match="call out of order"):      # no kept draws
        e0.draws_logpdf([2])
    e0.set_draws(np.ones((1, 3, 8)))
    with pytest.raises(RuntimeError, match="invalid argument"):
        e0.draws_logpdf([3])
    with pytest.raises(mamba.ArgumentError):
        mamba.Chains(np.ones((1, 3, 8)), ml.monitor_names, 1, 1, np.arange(1, 9), ml, None).dic()


def test_independent_of_the_sweep_kernel(mamba, monkeypatch, line_ref):
    """With the hipRTC-specialised sweep kernel active the logpdf kernel is the same interpreter."""
    v, _ = line_ref
    m, V = ir_line(mamba, v.shape[2])
    ej = ir_engine(mamba, monkeypatch, m, V, jit=True)
    ej.set_draws(v)
    keys = m.keys("stochastic")
    a = ej.draws_logpdf(ids_of(mamba, m, keys))
    m2, V2 = ir_line(mamba, v.shape[2])
    ei = ir_engine(mamba, monkeypatch, m2, V2, jit=False)
    ei.set_draws(v)
    assert np.array_equal(a, ei.draws_logpdf(ids_of(mamba, m2, keys)))
