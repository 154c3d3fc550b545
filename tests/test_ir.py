"""Node IR on the CPU: the lowering of Mamba Model DAGs, the oracle's
restatement of the IR semantics pinned against (i) the hand-lowered line and rats models,
(ii) an independent scipy evaluation of logpdf! (simulation.jl:77-90) for every supported
family and transform, (iii) libm lgamma, and the Calculus forward-difference gradient."""
import math

import numpy as np
import pytest
from scipy import stats
from scipy.special import expit, gammaln

RATS_BLOCKS = None


def ir_line(mamba, scheme):
    m = mamba.ir.line_model()
    m.setinputs(mamba.model.LINE_DATA)
    return m.setsamplers(scheme)


def test_lgamma_vs_libm(oracle):
    xs = np.concatenate([np.geomspace(1e-3, 1e4, 400), [0.5, 1.0, 1.5, 2.0, 2.5, 9.999, 10.0, 10.001]])
    for x in xs:
        want = math.lgamma(x)
        assert oracle.L.orc_lgamma(x) == pytest.approx(want, rel=1e-14, abs=1e-14), x


def test_ir_line_equals_hand_lowered_line(mamba, oracle):
    scheme = [mamba.AMWG(["beta", "s2"], 1.0), mamba.Slice("s2", 3.0)]
    m = ir_line(mamba, scheme)
    init = mamba.model.line_init_matrix(16, seed=3)
    V = m.init_matrix([{"y": [1.0, 3, 3, 3, 5], "beta": init[k, :2], "s2": init[k, 2]} for k in range(16)], 16)
    h = mamba.line().setinputs(mamba.model.LINE_DATA).setsamplers(scheme)
    np.testing.assert_array_equal(V, init)
    for k in range(16):
        x = np.array([V[k, 0], V[k, 1], np.log(V[k, 2])])
        assert oracle.block_logpdf(m, V[k], 0, x) == pytest.approx(oracle.block_logpdf(h, init[k], 0, x), rel=1e-13)
        assert oracle.block_logpdf(m, V[k], 1, [V[k, 2]]) == pytest.approx(
            oracle.block_logpdf(h, init[k], 1, [V[k, 2]]), rel=1e-13)
    assert m.monitor_names == ["beta[1]", "beta[2]", "s2"]


def test_ir_rats_equals_hand_lowered_rats(mamba, oracle):
    scheme = mamba.model.rats_scheme_reference()
    m = mamba.ir.rats_model().setinputs(mamba.ir.rats_inputs()).setsamplers(scheme)
    h = mamba.rats().setinputs(mamba.model.RATS_DATA).setsamplers(scheme)
    init = mamba.model.rats_init_ls(8, seed=4)
    # canonical orders: IR = declaration order (alpha, mu_alpha, s2_alpha, beta, mu_beta, s2_beta, s2_c)
    names = ["s2_c", "alpha", "mu_alpha", "s2_alpha", "beta", "mu_beta", "s2_beta"]
    sl = {"s2_c": slice(0, 1), "alpha": slice(1, 31), "mu_alpha": slice(31, 32), "s2_alpha": slice(32, 33),
          "beta": slice(33, 63), "mu_beta": slice(63, 64), "s2_beta": slice(64, 65)}
    inits = [{**{n: init[k, sl[n]] for n in names}, "y": mamba.model.RATS_Y} for k in range(8)]
    V = m.init_matrix(inits, 8)
    assert m.monitor_names == ["alpha0", "mu_beta", "s2_c"]
    rng = np.random.default_rng(1)
    for k in range(8):
        for b, s in enumerate(scheme):
            xh = np.concatenate([init[k, sl[p]] for p in s.params])
            xh = xh + rng.normal(0, 0.05, xh.size) * np.abs(xh)
            lp_h = oracle.block_logpdf(h, init[k], b, np.log(xh) if s.kind == mamba.abi.MMB_SAMPLER_AMWG and
                                       s.params[0].startswith("s2") else xh)
            lp_i = oracle.block_logpdf(m, V[k], b, xh)
            assert lp_i == pytest.approx(lp_h, rel=1e-12), (k, s)


# ---- every family and transform against scipy (the reference's logpdf! semantics) ----------

def zoo(mamba):
    ir = mamba.ir
    return ir.Model(
        obs_bin=ir.Stochastic(1, lambda nn, p: ir.Binomial(nn, p), False),
        obs_poi=ir.Stochastic(1, lambda lam, t: ir.Poisson(lam * t), False),
        obs_ber=ir.Stochastic(1, lambda p: ir.Bernoulli(p[1]), False),
        p=ir.Stochastic(1, lambda a, b: ir.Beta(a, b)),
        lam=ir.Stochastic(1, lambda g, th: ir.Gamma(g, th)),
        g=ir.Stochastic(lambda: ir.Exponential(2.0)),
        th=ir.Stochastic(lambda: ir.InverseGamma(3.0, 2.0)),
        a=ir.Stochastic(lambda: ir.Uniform(0.5, 4.0)),
        b=ir.Stochastic(lambda m0: ir.Normal(m0, 2.0)),
        m0=ir.Stochastic(lambda: ir.Normal(3.0, 1.0)))


ZOO_DATA = {"nn": [10.0, 12, 7, 20], "t": [1.0, 2.5, 0.5, 4.0, 1.5]}
ZOO_FIXED = {"obs_bin": [3.0, 0, 7, 11], "obs_poi": [0.0, 4, 1, 9, 2], "obs_ber": [1.0, 0, 1]}


def zoo_inits(rng, K):
    """Initial values of K zoo chains, every node inside its support."""
    inits = []
    for k in range(K):
        inits.append({**ZOO_FIXED, "p": rng.uniform(0.05, 0.95, 4), "lam": rng.gamma(2.0, 1.0, 5),
                      "g": rng.gamma(2.0, 1.0), "th": rng.gamma(2.0, 1.0), "a": rng.uniform(0.6, 3.9),
                      "b": rng.normal(3, 1), "m0": rng.normal(3, 1)})
    return inits


def zoo_ref_lp(blockparams, v, transform):
    """logpdf!(m, x, block, transform) by scipy: params \\ targets, then targets."""
    p, lam, g, th, a, b, m0 = v["p"], v["lam"], v["g"], v["th"], v["a"], v["b"], v["m0"]
    node = {
        "obs_bin": lambda: stats.binom.logpmf(ZOO_FIXED["obs_bin"], ZOO_DATA["nn"], p).sum(),
        "obs_poi": lambda: stats.poisson.logpmf(ZOO_FIXED["obs_poi"], lam * np.asarray(ZOO_DATA["t"])).sum(),
        "obs_ber": lambda: stats.bernoulli.logpmf(ZOO_FIXED["obs_ber"], p[0]).sum(),
        "p": lambda: (stats.beta.logpdf(p, a, b) + (np.log(p * (1 - p)) if tr("p") else 0)).sum(),
        "lam": lambda: (stats.gamma.logpdf(lam, g, scale=th) + (np.log(lam) if tr("lam") else 0)).sum(),
        "g": lambda: stats.expon.logpdf(g, scale=2.0) + (np.log(g) if tr("g") else 0),
        "th": lambda: stats.invgamma.logpdf(th, 3.0, scale=2.0) + (np.log(th) if tr("th") else 0),
        "a": lambda: stats.uniform.logpdf(a, 0.5, 3.5) + (np.log((a - 0.5) * (4 - a) / 3.5) if tr("a") else 0),
        "b": lambda: stats.norm.logpdf(b, m0, 2.0),
        "m0": lambda: stats.norm.logpdf(m0, 3.0, 1.0),
    }
    children = {"p": ["obs_bin", "obs_ber"], "lam": ["obs_poi"], "g": ["lam"], "th": ["lam"], "a": ["p"],
                "b": ["p"], "m0": ["b"]}

    def tr(n):
        return transform and n in blockparams

    targets = {c for q in blockparams for c in children[q]}
    order = ["obs_bin", "obs_poi", "obs_ber", "p", "lam", "g", "th", "a", "b", "m0"]
    topo = ["g", "th", "a", "m0", "lam", "b", "obs_poi", "p", "obs_bin", "obs_ber"]
    assert set(topo) == set(order)
    lp = 0.0
    for n in [q for q in blockparams if q not in targets] + [t for t in topo if t in targets]:
        lp += float(node[n]())
    return lp


def test_ir_families_vs_scipy(mamba, oracle):
    m = zoo(mamba).setinputs(ZOO_DATA)
    schemes = [mamba.AMWG(["p", "a"], 0.1), mamba.Slice(["lam", "g", "th"], 1.0, transform=True),
               mamba.Slice(["b", "m0"], 1.0), mamba.NUTS(["g", "th", "lam"])]
    m.setsamplers(schemes)
    rng = np.random.default_rng(7)
    inits = zoo_inits(rng, 6)
    V = m.init_matrix(inits, 6)
    names = ["p", "lam", "g", "th", "a", "b", "m0"]
    off = {n: m.nodes[n].offset for n in names}
    ln = {n: m.nodes[n].dim for n in names}
    links = {"p": (expit, lambda x: np.log(x / (1 - x))), "lam": (np.exp, np.log), "g": (np.exp, np.log),
             "th": (np.exp, np.log), "a": (lambda y: 3.5 * expit(y) + 0.5, lambda x: np.log((x - 0.5) / (4 - x))),
             "b": (lambda y: y, lambda x: x), "m0": (lambda y: y, lambda x: x)}
    for k in range(6):
        vals = {n: V[k, off[n]:off[n] + ln[n]] for n in names}
        vals = {n: (v if ln[n] > 1 else float(v[0])) for n, v in vals.items()}
        for bi, s in enumerate(schemes):
            trf = s.kind != mamba.abi.MMB_SAMPLER_SLICE or bool(s.transform)
            new = {n: vals[n] * (1.0 + rng.normal(0, 0.02, np.shape(vals[n]))) for n in s.params}
            x = np.concatenate([np.atleast_1d(links[n][1](new[n]) if trf else new[n]) for n in s.params])
            got = oracle.block_logpdf(m, V[k], bi, x)
            v2 = dict(vals)
            v2.update({n: (np.atleast_1d(links[n][0](links[n][1](np.asarray(new[n])))) if trf else
                           np.atleast_1d(new[n])) for n in s.params})
            v2 = {n: (np.asarray(v) if np.size(v) > 1 else float(np.ravel(v)[0])) for n, v in v2.items()}
            want = zoo_ref_lp(s.params, v2, trf)
            assert got == pytest.approx(want, rel=1e-11, abs=1e-10), (k, s.params)
    # out of support -> -Inf, and the early exit leaves it there
    x = np.array([0.5, 0.5, 0.5, 5.0])   # a = 5 is outside Uniform(0.5, 4) (AMWG block uses link: use Slice)
    ms = zoo(mamba).setinputs(ZOO_DATA).setsamplers([mamba.Slice(["p", "a"], 1.0)])
    Vs = ms.init_matrix(inits, 1)
    assert oracle.block_logpdf(ms, Vs[0], 0, x) == -np.inf


def test_ir_forward_difference_gradient(mamba, oracle):
    m = mamba.ir.surgical_model().setinputs(mamba.ir.SURGICAL)
    m.setsamplers([mamba.NUTS("b"), mamba.Slice(["mu", "s2"], 1.0)])
    inits = [{"r": mamba.ir.SURGICAL["r"], "b": np.linspace(-3, -2, 12), "s2": 0.3, "mu": -2.5}]
    V = m.init_matrix(inits, 1)
    x = np.linspace(-3.2, -1.9, 12)
    lp, g = oracle.block_logpdf(m, V[0], 0, x, grad=True)
    assert lp == oracle.block_logpdf(m, V[0], 0, x)
    for k in range(12):  # Calculus :forward, epsilon = sqrt(eps) * max(1, |x|), bit for bit
        e = 2.0 ** -26 * max(1.0, abs(x[k]))
        xp = x.copy()
        xp[k] = x[k] + e
        assert g[k] == (oracle.block_logpdf(m, V[0], 0, xp) - lp) / e
    # against the analytic gradient (loose: forward differences)
    p = expit(x)
    mu, s2 = -2.5, 0.3
    r, n = np.asarray(mamba.ir.SURGICAL["r"], float), np.asarray(mamba.ir.SURGICAL["n"], float)
    ga = r - n * p - (x - mu) / s2
    np.testing.assert_allclose(g, ga, rtol=1e-5, atol=1e-4)


def test_ir_lowering_structure(mamba):
    m = mamba.ir.seeds_model().setinputs(mamba.ir.SEEDS)
    m.setsamplers([mamba.AMM(["alpha0", "alpha1", "alpha2", "alpha12"], 0.01 * np.eye(4)), mamba.AMWG("b", 0.01),
                   mamba.AMWG("s2", 0.1)])
    m.init_matrix(mamba.ir.seeds_inits(), 2)
    ir = m.ir()
    assert m.nvalues == 4 + 21 + 1
    assert m.monitor_names == ["alpha0", "alpha1", "alpha2", "alpha12", "s2"]
    ids = {n: i for i, n in enumerate(m.order)}
    terms = [[ir.blocks[b].term[t] for t in range(ir.blocks[b].nterms)] for b in range(3)]
    # params \ targets in block order (their own priors), then the targets (simulation.jl:82-88)
    assert terms[0] == [ids[a] for a in ("alpha0", "alpha1", "alpha2", "alpha12")] + [ids["r"]]
    assert [s.targets for s in m.samplers] == [["r"], ["r"], ["b"]]
    assert terms[1] == [ids["b"], ids["r"]] and terms[2] == [ids["s2"], ids["b"]]
    assert [ir.blocks[2].trans[t] for t in range(2)] == [1, 0]


def test_ir_lowering_errors(mamba):
    ir = mamba.ir
    m = ir.seeds_model().setinputs(ir.SEEDS)
    with pytest.raises(mamba.ArgumentError, match="Gibbs"):
        m.setsamplers([mamba.Gibbs("s2")])
    with pytest.raises(mamba.ArgumentError, match="not a Stochastic node"):
        m.setsamplers([mamba.AMWG("nope", 1.0)])
    m.setsamplers([mamba.AMWG("r", 1.0)])
    with pytest.raises(mamba.ArgumentError, match="cannot be sampled"):
        m.init_matrix(ir.seeds_inits(), 2)
    with pytest.raises(mamba.ArgumentError, match="missing initial value"):
        m.setsamplers([mamba.AMWG("s2", 1.0)]).init_matrix([{"s2": 1.0}], 1)
    big = ir.Model(v=ir.Stochastic(1, lambda: ir.Normal(0, 1)))
    big.setinputs({}).setsamplers([mamba.AMWG("v", 1.0)])
    with pytest.raises(mamba.ArgumentError, match="at most 32"):
        big.init_matrix([{"v": np.zeros(40)}], 1)
    bad = ir.Model(v=ir.Stochastic(1, lambda s: ir.Uniform(0, s)), s=ir.Stochastic(lambda: ir.Gamma(1, 1)))
    bad.setinputs({}).setsamplers([mamba.AMWG("v", 1.0), mamba.AMWG("s", 1.0)])
    with pytest.raises(mamba.ArgumentError, match="Uniform bounds"):
        bad.init_matrix([{"v": np.ones(3), "s": 2.0}], 1)
    mm = ir.Model(y=ir.Stochastic(1, lambda mu, x: ir.MvNormal(mu * x, 1.0), False),
                  mu=ir.Stochastic(1, lambda: ir.Normal(0, 1)))
    mm.setinputs({"x": [1.0, 2, 3]}).setsamplers([mamba.AMWG("mu", 1.0)])
    with pytest.raises(mamba.ArgumentError, match="length"):
        mm.init_matrix([{"y": [1.0, 2, 3], "mu": [0.0, 1.0]}], 1)
    # code-word operands are 24 bits: a pool offset >= 2^24 would carry into the opcode
    W = mamba.ir._Lowering.word
    assert W(5, (1 << 24) - 1) == (5 << 24) | 0xffffff
    for bad_arg in (1 << 24, -1):
        with pytest.raises(mamba.ArgumentError, match="24 bits"):
            W(5, bad_arg)


def test_ir_create_validates_before_touching_the_device(mamba):
    """mmb_create_ir checks every code word / range on the host (no GPU here)."""
    import ctypes as C
    lib = mamba.abi.lib()
    m = mamba.ir.pumps_model().setinputs(mamba.ir.PUMPS)
    m.setsamplers([mamba.Slice(["alpha", "beta"], 1.0, mamba.Univariate), mamba.Slice("theta", 1.0, mamba.Univariate)])
    m.init_matrix([{"y": mamba.ir.PUMPS["y"], "alpha": 1.0, "beta": 1.0, "theta": np.ones(10)}], 1)
    h = C.c_void_p()
    sp = m.spec()
    assert lib.mmb_create(C.byref(sp), 0, C.byref(h)) == -1            # IR needs mmb_create_ir
    ir = m.ir()
    keep = m._ir_keep["code"].copy()
    try:
        m._ir_keep["code"][0] = (3 << 24) | 1000                        # VALI out of the state row
        assert lib.mmb_create_ir(C.byref(sp), C.byref(ir), 0, C.byref(h)) == -1
        assert b"invalid code" in lib.mmb_last_error(None)
    finally:
        m._ir_keep["code"][:] = keep
    sp.blocks[0].sampler = mamba.abi.MMB_SAMPLER_GIBBS
    assert lib.mmb_create_ir(C.byref(sp), C.byref(ir), 0, C.byref(h)) == -2


def _jit_source(mamba, m):
    import ctypes as C
    lib = mamba.abi.lib()
    spec, irm = m.spec(), m.ir()
    n = lib.mmb_ir_jit_source_text(C.byref(spec), C.byref(irm), None, 0)
    buf = C.create_string_buffer(n + 1)
    lib.mmb_ir_jit_source_text(C.byref(spec), C.byref(irm), buf, n + 1)
    return buf.value.decode()


def test_ir_specialised_source_is_straight_line(mamba):
    """mmb_create_ir's specialisation (csrc/ir_jit.cpp): the rats model with the reference scheme
    as HIP source -- y's MvNormal over the 150 observations with its mean alpha[rat] + beta[rat] *
    (x[j] - xbar) as four statements (two gathers, a data load, a multiply-add pair in the
    interpreter's order), one function per node and one case per block, no code-word dispatch,
    the sweep kernel instantiated for the scheme's sampler kinds only (Slice + AMWG)."""
    ir = mamba.ir
    m = ir.rats_model().setinputs(ir.rats_inputs()).setsamplers(mamba.model.rats_scheme_reference())
    m.init_matrix([{**mamba.model.RATS_INITS[k % 2], "y": mamba.model.RATS_Y} for k in range(2)], 2)
    src = _jit_source(mamba, m)
    assert "ir_code" not in src and "mmb_jit_block_lp" in src
    assert src.count("case ") >= len(m.samplers)
    kinds = 0
    for s in m.samplers:
        kinds |= 1 << s.kind
    assert f"sweep_body<MMB_MODEL_IR, {kinds}u>" in src
    # the y node's mean: gather alpha, gather beta, the data column, t3 * t4, t2 + t5
    assert "const double t5 = t3 * t4;" in src and "const double t6 = t2 + t5;" in src
    assert "d_iso(150, sig, ss)" in src


def test_ir_specialised_kernel_compiles_without_a_device(mamba):
    """hipRTC compiles the specialised kernel on the CPU build host (mmb_ir_jit_prebuild: the
    same validation as mmb_create_ir, then compile into the code-object cache)."""
    import ctypes as C
    ir = mamba.ir
    m = ir.line_model().setinputs(mamba.model.LINE_DATA).setsamplers([mamba.AMWG(["beta", "s2"], 1.0)])
    v = mamba.model.line_init_matrix(2, seed=1)
    m.init_matrix([{"y": [1.0, 3, 3, 3, 5], "beta": v[k, :2], "s2": v[k, 2]} for k in range(2)], 2)
    lib = mamba.abi.lib()
    buf = C.create_string_buffer(8192)
    rc = lib.mmb_ir_jit_prebuild(C.byref(m.spec()), C.byref(m.ir()), buf, len(buf))
    assert rc == 0, buf.value.decode()
    assert buf.value.decode().startswith(("cache hit", "compiled in"))


# ---------------------------------------------------------------- Gibbs closures (ABI 10)
def _line_gibbs_s2(ir):
    """doc/tutorial/line.jl:38-45, Gibbs_s2: rand(InverseGamma(length(y)/2 + shape(s2.distr),
    sumabs2(y - mu)/2 + scale(s2.distr))) with the prior InverseGamma(0.001, 0.001)."""
    return ir.Sampler(["s2"], lambda mu, y: ir.rand(ir.InverseGamma(ir.length(y) / 2.0 + 0.001,
                                                                    ir.sumabs2(y - mu) / 2.0 + 0.001)))


def test_ir_gibbs_closures_lowering(mamba):
    """User Sampler(params, f) closures (sampler.jl:20-24) are traced into node-IR Gibbs blocks:
    the conjugate family, one reduction per sum()/sumabs2() over its element count (gathers
    included: rats' y - (alpha[rat] + beta[rat] Xm) over 150 elements), and the constant Gamma
    shapes folded into one CONST word (so the kernel draws those variates with the iteration's
    others)."""
    ir, abi = mamba.ir, mamba.abi
    m = ir.rats_model().setinputs(ir.rats_inputs()).setsamplers(ir.rats_scheme_gibbs_amm())
    m.init_matrix(ir.rats_inits_ls(4, seed=1), 4)
    I, code, consts = m.ir(), m._ir_keep["code"], m._ir_keep["consts"]
    fam = [I.blocks[b].gibbs_family for b in range(7)]
    assert fam == [abi.MMB_IR_INVGAMMA, 0, abi.MMB_IR_NORMAL, abi.MMB_IR_INVGAMMA, 0, abi.MMB_IR_NORMAL,
                   abi.MMB_IR_INVGAMMA]
    assert [I.blocks[b].nred for b in range(7)] == [1, 0, 1, 1, 0, 1, 1]
    assert [I.blocks[b].red_len[0] for b in (0, 2, 3, 5, 6)] == [150, 30, 30, 30, 30]
    for b, a in ((0, 0.001 + 150 / 2), (3, 0.001 + 30 / 2), (6, 0.001 + 30 / 2)):
        pc = I.blocks[b].gibbs_expr[0]
        assert code[pc] >> 24 == abi.IR_OP["const"] and code[pc + 1] == 0 and consts[code[pc] & 0xffffff] == a
    # the scale expression reads the reduction through value slot nvalues + 0
    pc = I.blocks[0].gibbs_expr[1]
    assert (abi.IR_OP["val"] << 24 | m.nvalues) in list(code[pc:pc + 8])


def test_ir_gibbs_closure_errors(mamba):
    ir = mamba.ir
    with pytest.raises(mamba.ArgumentError, match="must return rand"):
        ir.Sampler(["s2"], lambda y: ir.InverseGamma(1.0, ir.sumabs2(y)))
    with pytest.raises(mamba.ArgumentError, match="must return rand"):
        ir.Sampler(["s2"], lambda y: ir.rand(ir.Beta(1.0, 2.0)))
    with pytest.raises(mamba.ArgumentError, match="traced closure"):
        ir.line_model().setsamplers([mamba.AMWG("beta", 1.0), mamba.Gibbs("s2")])
    m = ir.line_model().setinputs(mamba.model.LINE_DATA)
    m.setsamplers([ir.Sampler(["beta"], lambda y: ir.rand(ir.Normal(ir.mean(y), 1.0))), _line_gibbs_s2(ir)])
    with pytest.raises(mamba.ArgumentError, match="one scalar node"):
        m.init_matrix([{"y": [1.0, 3, 3, 3, 5], "beta": [0.0, 0.0], "s2": 1.0}], 1)
    m = ir.line_model().setinputs(mamba.model.LINE_DATA)
    m.setsamplers([mamba.AMWG("beta", 1.0), ir.Sampler(["s2"], lambda mu, y: ir.rand(ir.InverseGamma(1.0, y - mu)))])
    with pytest.raises(mamba.ArgumentError, match="not a scalar"):
        m.init_matrix([{"y": [1.0, 3, 3, 3, 5], "beta": [0.0, 0.0], "s2": 1.0}], 1)
    m = ir.line_model().setinputs(mamba.model.LINE_DATA)
    m.setsamplers([mamba.AMWG("beta", 1.0), ir.Sampler(["s2"], lambda y: ir.rand(ir.InverseGamma(1.0, ir.sum(
        ir.sum(y)))))])
    with pytest.raises(mamba.ArgumentError, match="inside a sum"):
        m.init_matrix([{"y": [1.0, 3, 3, 3, 5], "beta": [0.0, 0.0], "s2": 1.0}], 1)


def test_ir_gibbs_closures_reproduce_hand_lowered_rats(mamba, oracle):
    """The traced closures of INTEGRATION.md §3 are the hand-lowered conjugate blocks of the
    headline scheme (models.h gibbs, oracle orc_gibbs): run through the oracle's IR restatement on
    the same inits and seeds, the whole Gibbs + AMM trajectory -- kept draws and final state --
    equals the hand-lowered model's to rounding (the closures' formulas round differently:
    sum/s2/prec against vv (sum/s2 + 0/var0)), every accept decision the same."""
    ir = mamba.ir
    K = 32
    m = ir.rats_model().setinputs(ir.rats_inputs()).setsamplers(ir.rats_scheme_gibbs_amm())
    V = m.init_matrix(ir.rats_inits_ls(K, seed=1), K)
    st = oracle.new_state(m, V)
    d = oracle.run(m, st, 200, burnin=100, thin=2, seed=42, nthreads=8)
    h = mamba.rats().setinputs(mamba.model.RATS_DATA).setsamplers(mamba.model.rats_scheme_gibbs_amm())
    sth = oracle.new_state(h, mamba.model.rats_init_ls(K, seed=1))
    dh = oracle.run(h, sth, 200, burnin=100, thin=2, seed=42, nthreads=8)
    assert m.monitor_names == ["alpha0", "mu_beta", "s2_c"]  # the hand-lowered order is reversed
    np.testing.assert_allclose(d[:, ::-1, :], dh, rtol=1e-10, atol=1e-10)


def test_ir_gibbs_closure_line_s2(mamba, oracle):
    """line.jl's Gibbs_s2 closure (a reduction over the Logical mu = beta[1] + beta[2] x) beside
    AMWG(beta): the oracle's IR restatement equals the hand-lowered line Gibbs(s2) to rounding
    (the IR sums the 5 squared residuals in lane partials + the butterfly, the hand-lowered
    block sequentially)."""
    ir = mamba.ir
    K = 16
    m = ir.line_model().setinputs(mamba.model.LINE_DATA).setsamplers([mamba.AMWG("beta", 1.0), _line_gibbs_s2(ir)])
    init = mamba.model.line_init_matrix(K, seed=3)
    V = m.init_matrix([{"y": [1.0, 3, 3, 3, 5], "beta": init[k, :2], "s2": init[k, 2]} for k in range(K)], K)
    st = oracle.new_state(m, V)
    d = oracle.run(m, st, 200, burnin=100, thin=1, seed=9, nthreads=8)
    h = mamba.line().setinputs(mamba.model.LINE_DATA).setsamplers([mamba.AMWG("beta", 1.0), mamba.Gibbs("s2")])
    sth = oracle.new_state(h, init)
    dh = oracle.run(h, sth, 200, burnin=100, thin=1, seed=9, nthreads=8)
    np.testing.assert_allclose(d, dh, rtol=1e-9, atol=1e-12)


# ---- the element layer (csrc/ir_math.h, as the oracle compiles it) against 50-digit references --------
def _fam_ids(mamba):
    a = mamba.abi
    return {"normal": a.MMB_IR_NORMAL, "invgamma": a.MMB_IR_INVGAMMA, "gamma": a.MMB_IR_GAMMA,
            "exponential": a.MMB_IR_EXPONENTIAL, "uniform": a.MMB_IR_UNIFORM, "beta": a.MMB_IR_BETA,
            "binomial": a.MMB_IR_BINOMIAL, "poisson": a.MMB_IR_POISSON, "bernoulli": a.MMB_IR_BERNOULLI}


def _elem(oracle, fid, x, a=None, b=None, ct=0.0, tr=False, lo=0.0, hi=0.0):
    return oracle.L.orc_ir_elem_lp(fid, x, 0.0 if a is None else a, 0.0 if b is None else b, ct, int(tr), lo, hi)


def binom_ct(n, k):
    """The host-computed constant of a Binomial observation, as ir.py's lowering forms it."""
    return math.lgamma(n + 1) - math.lgamma(k + 1) - math.lgamma(n - k + 1)


def test_family_ref_vs_scipy():
    """tests/ir_family_ref.py (mpmath, 50 digits) against scipy.stats at interior points of all ten
    families, with and without the Jacobian.  Bound: 1e-13 M -- scipy evaluates the same sums of
    at most six terms in doubles from gammaln / xlogy / log1p, each good to a few ulps of its own
    term, so ~1e3 ulps (2^-53) of the term scale M is scipy's accuracy with room to spare, and
    four orders tighter than what the kernels are held to."""
    import ir_family_ref as R
    rng = np.random.default_rng(11)
    worst = 0.0

    def cmp(got, want):
        nonlocal worst
        v, M = got
        err = abs(float(v - R.mp.mpf(float(want))))
        worst = max(worst, err / M)
        assert err <= 1e-13 * M, (float(v), want, err, M)

    for _ in range(40):
        a, b = float(rng.gamma(2.0, 1.5)), float(rng.gamma(2.0, 1.5))
        x = float(rng.gamma(2.0, 1.0))
        u = float(rng.uniform(0.01, 0.99))
        z, mu = float(rng.normal(0, 3)), float(rng.normal(0, 2))
        for tr in (False, True):
            j = math.log(x) if tr else 0.0
            cmp(R.logpdf("gamma", x, a, b, tr), stats.gamma.logpdf(x, a, scale=b) + j)
            cmp(R.logpdf("invgamma", x, a, b, tr), stats.invgamma.logpdf(x, a, scale=b) + j)
            cmp(R.logpdf("exponential", x, a, tr=tr), stats.expon.logpdf(x, scale=a) + j)
            cmp(R.logpdf("beta", u, a, b, tr), stats.beta.logpdf(u, a, b) + (math.log(u * (1 - u)) if tr else 0.0))
            w = 0.5 + 3.5 * u
            cmp(R.logpdf("uniform", w, tr=tr, lo=0.5, hi=4.0),
                stats.uniform.logpdf(w, 0.5, 3.5) + (math.log((w - 0.5) * (4.0 - w) / 3.5) if tr else 0.0))
            cmp(R.logpdf("normal", z, mu, b, tr), stats.norm.logpdf(z, mu, b))
        n = int(rng.integers(1, 40))
        k = int(rng.integers(0, n + 1))
        cmp(R.logpdf("binomial", k, n, u), stats.binom.logpmf(k, n, u))
        cmp(R.logpdf("poisson", k, x), stats.poisson.logpmf(k, x))
        cmp(R.logpdf("bernoulli", k % 2, u), stats.bernoulli.logpmf(k % 2, u))
        xs, ms = rng.normal(0, 2, 5), rng.normal(0, 2, 5)
        cmp(R.logpdf("mvnormal", xs, ms, b), stats.norm.logpdf(xs, ms, b).sum())
    print("worst |ref - scipy| / M =", worst)
    # the support rule and the boundary conventions
    assert R.logpdf("gamma", -1.0, 2.0, 1.0)[0] == R.NINF and R.logpdf("beta", float("nan"), 2.0, 1.0)[0] == R.NINF
    assert R.logpdf("gamma", 0.0, 1.0, 2.0)[0] == -R.mp.log(2) and R.logpdf("gamma", 0.0, 0.5, 2.0)[0] == R.INF
    assert R.logpdf("gamma", 0.0, 1.0, 2.0, True)[0] == R.NINF
    assert R.mp.isnan(R.logpdf("gamma", 0.0, 0.5, 2.0, True)[0])


# worst |mmb_lgamma - mpmath.loggamma| / (|(z - 1/2) log z| + z) over test_lgamma_vs_mpmath's grid outside
# [1e-3, 1e4], measured on the oracle build: 6.58e-16 (three ulps of the Stirling terms' size)
LGAMMA_MEASURED = 6.6e-16


def test_lgamma_vs_mpmath(oracle):
    """mmb_lgamma (the oracle's build of ir_math.h) against mpmath.loggamma over
    geomspace(1e-300, 1e300) and around 1, 2 and 10.  On [1e-3, 1e4] the bound of
    test_lgamma_vs_libm (rel 1e-14, abs 1e-14) holds against the 50-digit value too.  Outside,
    the error is taken relative to M = |(z - 1/2) log z| + z: the worst over this grid measured
    6.58e-16 (LGAMMA_MEASURED); 4x that, 2.64e-15 M, is asserted."""
    import ir_family_ref as R
    xs = np.concatenate([np.geomspace(1e-300, 1e300, 2401), np.geomspace(1e-3, 1e4, 400),
                         [0.5, 1.0, 1.5, 2.0, 2.5, 9.999, 10.0, 10.001]])
    worst_out = 0.0
    for x in xs:
        x = float(x)
        got = oracle.L.orc_lgamma(x)
        want = R.mp.loggamma(R.mp.mpf(x))
        if 1e-3 <= x <= 1e4:
            assert got == pytest.approx(float(want), rel=1e-14, abs=1e-14), x
        else:
            e = float(abs(R.mp.mpf(got) - want)) / float(R.lgamma_scale(x))
            worst_out = max(worst_out, e)
            assert e <= 4 * LGAMMA_MEASURED, (x, got, float(want), e)
    print("worst |lgamma - mpmath| / M outside [1e-3, 1e4] =", worst_out)
    assert oracle.L.orc_lgamma(0.0) == math.inf and math.isnan(oracle.L.orc_lgamma(-1.0))


def test_ir_elem_edges_vs_ref(mamba, oracle):
    """Every point of the edge grid (ir_family_ref.edge_grid, PROBS, RATES), with and without the
    transform, on the oracle's element layer: the class (nan / +inf / -inf / finite) is the
    reference's and finite values lie within 1e-12 M + 1e-13 -- the assertion the device test
    (test_gpu_ir_families.py) makes of modelstats.hip at the same points."""
    import ir_family_ref as R
    F = _fam_ids(mamba)
    n = 0
    for fam in ("beta", "gamma", "invgamma", "exponential", "normal", "uniform"):
        lo, hi = (R.UNIFORM_LO, R.UNIFORM_HI) if fam == "uniform" else (0.0, 0.0)
        for x, a, b in R.edge_grid(fam):
            for tr in (False, True):
                got = _elem(oracle, F[fam], x, a, b, tr=tr, lo=lo, hi=hi)
                R.check(got, *R.logpdf(fam, x, a, b, tr, lo, hi), where=(fam, x, a, b, tr), tr=tr)
                n += 1
    for k, nn in ((3.0, 10.0), (0.0, 12.0), (7.0, 7.0), (11.0, 20.0)):
        for p in R.PROBS:
            got = _elem(oracle, F["binomial"], k, nn, p, ct=binom_ct(nn, k))
            R.check(got, *R.logpdf("binomial", k, nn, p), where=("binomial", k, nn, p))
    for k in (0.0, 4.0, 9.0):
        for lam in R.RATES:
            for t in (1.0, 2.5):
                got = _elem(oracle, F["poisson"], k, lam * t, ct=-math.lgamma(k + 1))
                R.check(got, *R.logpdf("poisson", k, lam * t), where=("poisson", k, lam * t))
    for x in (0.0, 1.0):
        for p in R.PROBS:
            R.check(_elem(oracle, F["bernoulli"], x, p), *R.logpdf("bernoulli", x, p), where=("bernoulli", x, p))
    assert n > 1400


def test_ir_boundary_values(mamba, oracle):
    """The densities at the support boundaries, where (a - 1) log x is 0 * -Inf: Beta at 0 (+Inf,
    log b, -Inf for a below, equal to and above 1), mirrored at 1, Gamma at 0 (+Inf, -log theta,
    -Inf); InverseGamma at 0; with the transform -Inf everywhere the density is not +Inf (and
    never NaN: a Slice shrink test !(lp < p0) accepts NaN)."""
    F = _fam_ids(mamba)
    e = lambda *a, **k: _elem(oracle, *a, **k)      # noqa: E731
    inf = math.inf
    # Beta(a, 3) at 0 and Beta(3, b) at 1
    assert e(F["beta"], 0.0, 0.5, 3.0) == inf and e(F["beta"], 0.0, 2.0, 3.0) == -inf
    assert e(F["beta"], 0.0, 1.0, 3.0) == pytest.approx(math.log(3.0), abs=1e-14)
    assert e(F["beta"], 1.0, 3.0, 0.5) == inf and e(F["beta"], 1.0, 3.0, 2.0) == -inf
    assert e(F["beta"], 1.0, 3.0, 1.0) == pytest.approx(math.log(3.0), abs=1e-14)
    assert e(F["beta"], 0.0, 1.0, 1.0) == pytest.approx(0.0, abs=1e-14)
    assert e(F["beta"], 1.0, 1.0, 1.0) == pytest.approx(0.0, abs=1e-14)
    # Gamma(k, 2) at 0
    assert e(F["gamma"], 0.0, 0.5, 2.0) == inf and e(F["gamma"], 0.0, 2.0, 2.0) == -inf
    assert e(F["gamma"], 0.0, 1.0, 2.0) == pytest.approx(-math.log(2.0), abs=1e-14)
    assert e(F["invgamma"], 0.0, 3.0, 2.0) == -inf
    for fam, x, a, b in (("beta", 0.0, 1.0, 1.0), ("beta", 1.0, 1.0, 1.0), ("beta", 0.0, 0.5, 3.0),
                         ("beta", 1.0, 3.0, 0.5), ("beta", 0.0, 2.0, 3.0), ("gamma", 0.0, 1.0, 2.0),
                         ("gamma", 0.0, 0.5, 2.0), ("gamma", 0.0, 2.0, 2.0), ("gamma", inf, 1.0, 2.0),
                         ("gamma", inf, 3.0, 2.0), ("invgamma", 0.0, 3.0, 2.0), ("invgamma", inf, 3.0, 2.0),
                         ("exponential", 0.0, 2.0, None), ("exponential", inf, 2.0, None)):
        assert e(F[fam], x, a, b, tr=True) == -inf, (fam, x, a, b)
    # block log densities through the links (the wide-Slice model): invlogit(40) is exactly 1,
    # invlogit(-800) and exp(-800) exactly 0, exp(800) is Inf
    m, V = wide_slice(mamba, 2)
    raw = wide_slice(mamba, 2, transform=False)[0]
    for y in (40.0, -800.0):
        assert oracle.block_logpdf(m, V[0], 0, [y, 0.0, 0.0, 0.0]) == -inf
    for y in (-800.0, 800.0):
        assert oracle.block_logpdf(m, V[0], 1, [y, 0.0, 0.0]) == -inf
    # no transform: p = 0 with 3 successes of 10, p = 1 with 7 failures, lam = 0 with 4 events
    # seen are impossible (-Inf, not NaN); p[3] = 1 with 7 of 7 and lam[1] = 0 with no event are not
    assert oracle.block_logpdf(raw, V[0], 0, [0.0, 0.5, 0.5, 0.5]) == -inf
    assert oracle.block_logpdf(raw, V[0], 0, [1.0, 0.5, 0.5, 0.5]) == -inf
    assert oracle.block_logpdf(raw, V[0], 1, [1.0, 0.0, 1.0]) == -inf
    assert math.isfinite(oracle.block_logpdf(raw, V[0], 0, [0.5, 0.0, 1.0, 0.5]))
    assert math.isfinite(oracle.block_logpdf(raw, V[0], 1, [0.0, 1.0, 1.0]))


WIDE_DATA = {"nn": [10.0, 12, 7, 20], "t": [1.0, 2.5, 0.5]}
WIDE_FIXED = {"obs_bin": [3.0, 0, 7, 11], "obs_poi": [0.0, 4, 1]}
# Window widths of the two Univariate Slice blocks on the link scale.  100 on logit(p) puts most
# first candidates beyond |y| = 37, where invlogit is exactly 0 or 1; 3000 on log(lam) beyond
# |y| = 746, where exp is exactly 0 or Inf.  Both are the widths the defect was found with: the
# fixed code needs ~10 shrinks per coordinate there, nowhere near MMB_SLICE_MAX_SHRINK, so
# neither was narrowed.
WIDE_W_P, WIDE_W_LAM = 100.0, 3000.0


def wide_slice(mamba, K, transform=True, seed=3):
    """p[1..4] ~ Beta(1, 1) with Binomial observations, lam[1..3] ~ Gamma(1, 2) with Poisson
    observations; two Univariate Slice blocks with windows far wider than the posterior."""
    ir = mamba.ir
    m = ir.Model(
        obs_bin=ir.Stochastic(1, lambda nn, p: ir.Binomial(nn, p), False),
        obs_poi=ir.Stochastic(1, lambda lam, t: ir.Poisson(lam * t), False),
        p=ir.Stochastic(1, lambda: ir.Beta(1.0, 1.0)),
        lam=ir.Stochastic(1, lambda: ir.Gamma(1.0, 2.0)))
    m.setinputs(WIDE_DATA)
    m.setsamplers([mamba.Slice("p", WIDE_W_P, mamba.Univariate, transform=transform),
                   mamba.Slice("lam", WIDE_W_LAM, mamba.Univariate, transform=transform)])
    rng = np.random.default_rng(seed)
    inits = [{**WIDE_FIXED, "p": rng.uniform(0.05, 0.95, 4), "lam": rng.gamma(2.0, 1.0, 3)} for _ in range(K)]
    return m, m.init_matrix(inits, K)


def test_ir_wide_slice_stays_inside(mamba, oracle):
    """Slice windows of width 100 (logit p) and 3000 (log lam) on Beta(1, 1) and Gamma(1, 2) priors:
    candidates land where the link saturates (p exactly 0 or 1, lam exactly 0 or Inf).  Their log
    density is -Inf, so they are shrunk away; when it was NaN (0 * -Inf) the shrink test
    !(lp < p0) accepted them and most of the run was NaN (this very run: 14 747 of the 17 920 kept
    values, after draws of p == 1 and lam == 0).  64 chains, 40 iterations, every iteration kept.
    Also caught here: a Poisson rate lam * t that overflows to Inf (k log Inf - Inf = NaN)."""
    m, V = wide_slice(mamba, 64)
    st = oracle.new_state(m, V)
    d = oracle.run(m, st, 40, burnin=0, thin=1, seed=17, nthreads=8)
    assert d.shape == (40, 7, 64)
    assert not np.isnan(d).any(), int(np.isnan(d).sum())
    assert np.isfinite(d).all()
    assert (d[:, :4, :] > 0).all() and (d[:, :4, :] < 1).all() and (d[:, 4:, :] > 0).all()
    # and the chains move: no coordinate of any chain sits still over the run
    assert (np.ptp(d, axis=0) > 0).all()


def test_oracle_refuses_samplers_it_does_not_restate(mamba, oracle):
    """oracle.c has no RWM update: run_chain would skip such a block, and a comparison against
    it would be against chains that never moved.  The binding raises instead."""
    m = mamba.ir.line_model().setinputs(mamba.model.LINE_DATA)
    m.setsamplers([mamba.RWM("beta", 1.0), mamba.AMWG("s2", 1.0)])
    v = mamba.model.line_init_matrix(2, seed=1)
    V = m.init_matrix([{"y": [1.0, 3, 3, 3, 5], "beta": v[k, :2], "s2": v[k, 2]} for k in range(2)], 2)
    with pytest.raises(NotImplementedError, match="does not restate"):
        oracle.new_state(m, V)
    tw = mamba.ir.line_model().setinputs(mamba.model.LINE_DATA).setsamplers([mamba.AMWG("beta", 1.0),
                                                                            mamba.AMWG("s2", 1.0)])
    tw.init_matrix([{"y": [1.0, 3, 3, 3, 5], "beta": v[k, :2], "s2": v[k, 2]} for k in range(2)], 2)
    st = oracle.new_state(tw, V)
    with pytest.raises(NotImplementedError, match="does not restate"):
        oracle.run(m, st, 1)
