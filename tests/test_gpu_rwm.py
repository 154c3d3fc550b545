"""RWM (src/samplers/rwm.jl:49-71) on the GPU: the line (one lane per chain), rats (32 lanes per
chain), node-IR interpreter and hipRTC-specialised kernels against the Python restatement of the
update (tests/rwm_ref.py) on identical Philox streams -- draws, final values, tune rows and the
update / accept counts identical, zero differing bits -- then mixed schemes, invariances and the
posteriors."""
import functools
import json
import os

import numpy as np
import pytest

import rwm_ref

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
PROPOSALS = ["Normal", "SymUniform", "SymTriangularDist", "Epanechnikov", "Biweight", "Triweight", "Cosine"]


def _mb():
    import _mamba_path
    return _mamba_path.load()


def _oracle():
    import oracle_lib
    return oracle_lib.Oracle()


# ---- models: make(scheme) -> (model, init matrix); the twin is make(twin_scheme(scheme))
def line_make(K, seed=123):
    def make(scheme):
        mb = _mb()
        m = mb.line().setinputs(mb.model.LINE_DATA).setsamplers(scheme)
        return m, mb.model.line_init_matrix(K, seed=seed)
    return make


def rats_make(K):
    def make(scheme):
        mb = _mb()
        m = mb.rats().setinputs(mb.model.RATS_DATA).setsamplers(scheme)
        return m, mb.model.rats_init_ls(K)
    return make


def ir_make(name, K):
    def make(scheme):
        mb = _mb()
        ir = mb.ir
        if name == "dyes":
            m = ir.dyes_model().setinputs(ir.dyes_inputs()).setsamplers(scheme)
            inits = [{"y": ir.DYES_Y, "theta": 1500, "s2_within": 1, "s2_between": 1, "mu": [1500] * 6} if k % 2 == 0
                     else {"y": ir.DYES_Y, "theta": 3000, "s2_within": 10, "s2_between": 10, "mu": [3000] * 6}
                     for k in range(K)]
        elif name == "rats":
            m = ir.rats_model().setinputs(ir.rats_inputs()).setsamplers(scheme)
            inits = ir.rats_inits_ls(K, seed=5)
        else:
            m = ir.line_model().setinputs(mb.model.LINE_DATA).setsamplers(scheme)
            v = mb.model.line_init_matrix(K)
            inits = [{"y": [1.0, 3, 3, 3, 5], "beta": v[k, :2], "s2": v[k, 2]} for k in range(K)]
        return m, m.init_matrix(inits, K)
    return make


def line_scheme(mb, prop="Normal"):
    return [mb.RWM("beta", [1.0, 0.4], prop), mb.RWM("s2", 1.5, prop)]


def rats_scheme(mb):
    """pure RWM on every rats block: the two 30-element vector blocks, a one-node and two two-node
    scalar blocks, four proposal families"""
    return [mb.RWM("s2_c", 0.3, mb.Cosine), mb.RWM("alpha", 1.0),
            mb.RWM(["mu_alpha", "s2_alpha"], [3.0, 0.5], mb.Triweight), mb.RWM("beta", 0.1, mb.SymUniform),
            mb.RWM(["mu_beta", "s2_beta"], [0.1, 0.5])]


def dyes_rwm(mb):
    return [mb.RWM("theta", 50, mb.Cosine), mb.RWM("mu", 50), mb.RWM(["s2_within", "s2_between"], 1.0)]


def dyes_scheme4(mb):  # doc/examples/dyes.jl:69-71
    return [mb.RWM("theta", 50.0, mb.Cosine), mb.RWM("mu", 50.0), mb.Slice(["s2_within", "s2_between"], 1000.0)]


def restatement(make, scheme, seed, chain_offset=0):
    mb = _mb()
    m, V = make(scheme)
    tw, _ = make(rwm_ref.twin_scheme(mb, scheme))
    return rwm_ref.Restatement(_oracle(), mb, m, tw, seed, chain_offset), m, V


def restate(make, scheme, seed, iters, burnin, thin, scales=None):
    """A whole pure-RWM run restated: (draws, final values, tune rows, stats, per-chain accepts)."""
    R, m, V = restatement(make, scheme, seed)
    vals = V.copy()
    sc = R.scales0(V.shape[0]) if scales is None else scales
    d = R.run(vals, iters, burnin=burnin, thin=thin, scales=sc)
    return d, vals, R.tune(sc, V.shape[0]), R.stats(), dict(R.chain_accepts)


def check_exact(eng, dg, ref):
    d, vals, tune, stats, _ = ref
    np.testing.assert_array_equal(dg, d)
    np.testing.assert_array_equal(eng.values(), vals)
    np.testing.assert_array_equal(eng.tune(), tune)
    got = eng.rwm_stats()
    assert {b: (v["updates"], v["accepts"]) for b, v in got.items()} == \
        {b: (v["updates"], v["accepts"]) for b, v in stats.items()}


# ---- 1. line, hand-lowered, pure RWM
@pytest.mark.parametrize("prop", PROPOSALS)
def test_line_rwm_exact(mamba, prop):
    """70 chains (a full 64-thread block and a ragged one), 40 iterations, burn-in 10, thin 2."""
    make = line_make(70)
    scheme = line_scheme(mamba, prop)
    ref = restate(make, scheme, 11, 40, 10, 2)
    m, V = make(scheme)
    eng = mamba.Engine(m)
    eng.init_chains(V, seed=11)
    dg = eng.run(40, burnin=10, thin=2)
    check_exact(eng, dg, ref)
    eng.close()


# ---- 2. rats, hand-lowered, pure RWM
@functools.lru_cache(maxsize=None)
def rats_ref():
    return restate(rats_make(19), rats_scheme(_mb()), 11, 60, 20, 2)


def run_rats(mamba, K=19, chain_offset=0, init=None, iters=60):
    m, V = rats_make(K)(rats_scheme(mamba))
    eng = mamba.Engine(m)
    eng.init_chains(V if init is None else init, chain_offset=chain_offset, seed=11)
    return eng, eng.run(iters, burnin=20, thin=2)


def test_rats_rwm_exact(mamba):
    """rats_init_ls(19): two workgroups of eight chains, a ragged one, an unpaired chain in its last
    wavefront; seed 11, 60 iterations.  Not vacuous: every block's acceptance in the restatement
    lies in [0.2, 0.8]."""
    ref = rats_ref()
    for b, v in ref[3].items():
        rate = v["accepts"] / v["updates"]
        print("block", b, "acceptance", rate)
        assert 0.2 <= rate <= 0.8, (b, rate)
    eng, dg = run_rats(mamba)
    check_exact(eng, dg, ref)
    eng.close()


# ---- 3. node IR, specialised and interpreter kernels
IR_CASES = {"dyes_rwm": ("dyes", dyes_rwm), "rats_rwm": ("rats", rats_scheme),
            # mixed schemes (test 4); listed here so that tools/jit_prebuild.py compiles them
            "dyes_scheme4": ("dyes", dyes_scheme4)}


def ir_models():
    """(label, model) of every node-IR model this file creates (tools/jit_prebuild.py)."""
    mb = _mb()
    return [(f"rwm_{k}", ir_make(name, 2)(sch(mb))[0]) for k, (name, sch) in sorted(IR_CASES.items())]


@functools.lru_cache(maxsize=None)
def ir_ref(case):
    name, sch = IR_CASES[case]
    return restate(ir_make(name, 96), sch(_mb()), 11, 60, 20, 2)


@pytest.mark.parametrize("kernel", ["specialised", "interpreter"])
@pytest.mark.parametrize("case", ["dyes_rwm", "rats_rwm"])
def test_ir_rwm_exact(mamba, case, kernel, monkeypatch):
    """96 chains, 60 iterations, burn-in 20, thin 2: the hipRTC-specialised kernel and the
    interpreter (MMB_IR_JIT=0) both equal the restatement."""
    if kernel == "interpreter":
        monkeypatch.setenv("MMB_IR_JIT", "0")
    name, sch = IR_CASES[case]
    ref = ir_ref(case)
    if case == "dyes_rwm":
        print("acceptance", {b: v["accepts"] / v["updates"] for b, v in ref[3].items()})
    m, V = ir_make(name, 96)(sch(mamba))
    eng = mamba.Engine(m)
    assert eng.ir_jit()[0] == (kernel == "specialised"), eng.ir_jit()
    eng.init_chains(V, seed=11)
    dg = eng.run(60, burnin=20, thin=2)
    check_exact(eng, dg, ref)
    eng.close()


# ---- 4. mixed schemes
def test_dyes_scheme4_mixed(mamba, monkeypatch):
    """dyes.jl:69-71 (RWM Cosine, RWM, Slice): theta and mu after one iteration equal the restatement
    (the RWM blocks precede the Slice block); over 60 iterations specialised == interpreter."""
    make = ir_make("dyes", 96)
    scheme = dyes_scheme4(mamba)
    R, m, V = restatement(make, scheme, 11)
    vals = V.copy()
    R.run(vals, 1, nblocks=2)
    out = {}
    for kernel in ("specialised", "interpreter"):
        if kernel == "interpreter":
            monkeypatch.setenv("MMB_IR_JIT", "0")
        m, V = make(dyes_scheme4(mamba))
        eng = mamba.Engine(m)
        assert eng.ir_jit()[0] == (kernel == "specialised"), eng.ir_jit()
        eng.init_chains(V, seed=11)
        eng.run(1, draws=False)
        v1 = eng.values()
        for p in ("theta", "mu"):
            n = m.nodes[p]
            np.testing.assert_array_equal(v1[:, n.offset:n.offset + n.dim], vals[:, n.offset:n.offset + n.dim])
        d = eng.run(59, burnin=20, thin=2)
        out[kernel] = (d, eng.values(), eng.tune(), eng.rwm_stats())
        eng.close()
    a, b = out["specialised"], out["interpreter"]
    for x, y in zip(a[:3], b[:3]):
        np.testing.assert_array_equal(x, y)
    assert a[3] == b[3] and a[3][0]["updates"] == 96 * 60


@pytest.mark.parametrize("second", ["slice", "nuts"])
def test_line_mixed(mamba, second):
    """[RWM(beta), Slice(s2)] and [RWM(beta), NUTS(s2)]: the line kernels that hold RWM next to the
    other kinds, without and with the gradient kinds; beta after iteration 1 equals the restatement."""
    def scheme():
        return [mamba.RWM("beta", [1.0, 0.4], mamba.Biweight),
                mamba.Slice("s2", 2.0) if second == "slice" else mamba.NUTS("s2")]
    make = line_make(70)
    R, m, V = restatement(make, scheme(), 11)
    vals = V.copy()
    R.run(vals, 1, nblocks=1)
    m, V = make(scheme())
    eng = mamba.Engine(m)
    eng.init_chains(V, seed=11)
    eng.run(1, draws=False)
    v1 = eng.values()
    np.testing.assert_array_equal(v1[:, :2], vals[:, :2])
    assert np.all(np.isfinite(v1)) and np.any(v1[:, 2] != V[:, 2])
    assert eng.rwm_stats()[0]["updates"] == 70
    eng.close()


# ---- 5. invariances, all exact
def test_chain_offset_split(mamba):
    """64 chains as one engine equal two engines with chain_offset 0 and 32."""
    V = mamba.model.rats_init_ls(64)
    e0, d0 = run_rats(mamba, 64, init=V)
    ea, da = run_rats(mamba, 32, init=V[:32])
    eb, db = run_rats(mamba, 32, chain_offset=32, init=V[32:])
    np.testing.assert_array_equal(d0, np.concatenate([da, db], axis=2))
    np.testing.assert_array_equal(e0.values(), np.concatenate([ea.values(), eb.values()], axis=0))
    s0, sa, sb = e0.rwm_stats(), ea.rwm_stats(), eb.rwm_stats()
    assert all(s0[b]["accepts"] == sa[b]["accepts"] + sb[b]["accepts"] for b in s0)
    for e in (e0, ea, eb):
        e.close()


def test_restart(mamba):
    """30 + 30 iterations through mcmc_restart equal 60."""
    def model():
        return mamba.line().setsamplers(line_scheme(mamba, mamba.SymTriangularDist))
    V = mamba.model.line_init_matrix(70)
    whole = mamba.mcmc(model(), mamba.model.LINE_DATA, V, 60, burnin=0, thin=2, chains=70, seed=11)
    part = mamba.mcmc(model(), mamba.model.LINE_DATA, V, 30, burnin=0, thin=2, chains=70, seed=11)
    part = mamba.mcmc_restart(part, 30)
    np.testing.assert_array_equal(part.value, whole.value)
    np.testing.assert_array_equal(part.engine.values(), whole.engine.values())
    assert part.engine.rwm_stats() == whole.engine.rwm_stats()


def test_sweep_parts(mamba, monkeypatch):
    """MMB_SWEEP_PARTS=3 equals 1 on the rats scheme."""
    monkeypatch.setenv("MMB_SWEEP_PARTS", "3")
    eng, dg = run_rats(mamba)
    check_exact(eng, dg, rats_ref())
    eng.close()


def test_zero_scale_chain(mamba):
    """A chain whose scale row is set to 0 through set_tune keeps its values for the whole run and
    counts every update as accepted (exp(0) = 1 > u); its neighbours are unchanged.  Chain 4 starts
    with its three variances at 1.0, which the log link returns exactly (log 1 = 0, exp 0 = 1)."""
    make = rats_make(19)
    m, V = make(rats_scheme(mamba))
    assert np.all(V[4, [0, 32, 64]] == 1.0)
    eng = mamba.Engine(m)
    eng.init_chains(V, seed=11)
    t = eng.tune()
    assert t.shape == (19, 1 + 30 + 2 + 30 + 2)
    t[4, :] = 0.0
    eng.set_tune(t)
    np.testing.assert_array_equal(eng.tune(), t)
    dg = eng.run(60, burnin=20, thin=2)
    vals = eng.values()
    np.testing.assert_array_equal(vals[4], V[4])
    ref = rats_ref()
    keep = np.arange(19) != 4
    np.testing.assert_array_equal(vals[keep], ref[1][keep])
    np.testing.assert_array_equal(dg[:, :, keep], ref[0][:, :, keep])
    # counts: the neighbours' accepts as in the reference run, chain 4's every update
    got = eng.rwm_stats()
    for b in range(5):
        others = ref[3][b]["accepts"] - ref[4][(b, 4)]
        assert got[b]["updates"] == 19 * 60 and got[b]["accepts"] == others + 60, (b, got[b])
    # and the restatement of the zero-scale run agrees with all of it
    R, _, _ = restatement(make, rats_scheme(mamba), 11)
    sc = R.scales0(19)
    for b in sc:
        sc[b][4, :] = 0.0
    row = V[4:5].copy()
    for it in range(1, 61):
        for b in range(5):
            assert R.update(row[0], b, 4, it, sc[b][4])
    np.testing.assert_array_equal(row[0], V[4])
    eng.close()


# ---- 6. statistical tests
def dyes_dispersed(mamba, K, seed=21):
    """dyes inits for fixed-scale samplers: the reference's two (dyes.jl:49-54: theta = 1500 | 3000, both
    variances 1 | 10), with mu = theta + N(0, 50^2) per batch in place of mu = theta exactly."""
    ir = mamba.ir
    rng = np.random.default_rng(seed)
    m = ir.dyes_model().setinputs(ir.dyes_inputs()).setsamplers(dyes_scheme4(mamba))
    inits = []
    for k in range(K):
        th, s2 = (1500.0, 1.0) if k % 2 == 0 else (3000.0, 10.0)
        inits.append({"y": ir.DYES_Y, "theta": th, "s2_within": s2, "s2_between": s2,
                      "mu": th + rng.normal(0.0, 50.0, 6)})
    return m, m.init_matrix(inits, K)


def test_dyes_scheme4_published(mamba):
    """dyes scheme4 (dyes.jl:69-71), 2048 chains at the published run length, against the
    reference's published summaries: the criterion of test_ir_published_summaries, |ours -
    published| within 5 published MCSE + 4 of our own SE.

    Inits.  The reference's inits start with mu == theta exactly, so sum (mu - theta)^2 = 0 and the
    first Slice draw of s2_between is ~ InverseGamma(3, 0.001): about 1e-3.  A scale-50 proposal of
    mu or theta then has next to no chance, and RWM adapts nothing (NUTS, which the published run
    used, adapts its step size and leaves): a chain that enters this neck stays for longer than the
    run.  The same degeneracy as the rats constant inits (model.rats_init_ls).  So mu starts dispersed
    around theta by the proposal's own scale, everything else as the reference has it.  Measured with
    the reference's inits instead (2048 chains, 2502:10000): theta 1521.69 +- 0.24 (chains from
    inits[0] 1516.72, from inits[1] 1526.66; published 1526.72), mu[2] 1522.58 (published 1527.91,
    tolerance 2.50) -- the same at 30002:60000 (theta 1516.69 | 1526.71), so not slow burn-in; the
    kernels equal the restatement bit for bit there too (test_dyes_scheme4_mixed).  With these inits:
    theta 1526.719 +- 0.061, both halves alike (1526.71 | 1526.72)."""
    g = json.load(open(os.path.join(GOLD, "ir_published.json")))["dyes"]
    pub = g["rows"]
    first, last = (int(t) for t in g["iterations"].split(":"))
    m, V = dyes_dispersed(mamba, 2048)
    eng = mamba.Engine(m)
    eng.init_chains(V, seed=2026)
    d = eng.run(last, burnin=first - 2, thin=2)
    print("acceptance", {b: v["rate"] for b, v in eng.rwm_stats().items()})
    seen = 0
    for j, nm in enumerate(m.monitor_names):
        if nm not in pub:
            continue
        seen += 1
        cm = d[:, j, :].mean(axis=0)
        est, se = float(cm.mean()), float(cm.std(ddof=1) / np.sqrt(cm.size))
        tol = 5.0 * pub[nm]["mcse"] + 4.0 * se
        print(nm, est, pub[nm]["mean"], tol)
        assert abs(est - pub[nm]["mean"]) < tol, (nm, est, pub[nm]["mean"], tol)
    assert seen == 9
    eng.close()


def test_line_posterior(mamba):
    """Line RWM, 2048 chains x 3000 iterations (first 500 dropped), against the exact posterior
    (tests/golden/line_posterior.json): means within 4 between-chain standard errors, the criterion
    the restatement itself meets on the CPU (tests/test_rwm.py)."""
    post = json.load(open(os.path.join(GOLD, "line_posterior.json")))
    K = 2048
    m, V = line_make(K)([mamba.RWM("beta", [1.0, 0.4]), mamba.RWM("s2", 1.5, mamba.Epanechnikov)])
    eng = mamba.Engine(m)
    eng.init_chains(V, seed=11)
    d = eng.run(3000, burnin=500, thin=1)
    print("acceptance", {b: v["rate"] for b, v in eng.rwm_stats().items()})
    for j, key in enumerate(["E_beta1", "E_beta2", "E_s2"]):
        cm = d[:, j, :].mean(axis=0)
        est, se = float(cm.mean()), float(cm.std(ddof=1) / np.sqrt(K))
        print(key, est, "+-", se, "exact", post[key])
        assert abs(est - post[key]) < 4.0 * se, (key, est, se, post[key])
    eng.close()
