"""DGS (src/samplers/dgs.jl:56-126) on the CPU: the constants, the constructor and every refusal of the
host, the lowered IR of the test models (tests/dgs_ref.py), the restatement against hand-computed
conditionals, and the observed-Binomial lowering pinned to what it was before discrete sampling."""
import ctypes as C
import hashlib
import math
import os
import re

import numpy as np
import pytest

import dgs_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lowered(mamba, name, scheme, K=4):
    m, inputs, inits = getattr(dgs_ref, name)(mamba.ir)
    m.setinputs(inputs).setsamplers(scheme)
    V = m.init_matrix(inits(K), K)
    return m, V


def words(m):
    return [int(w) for w in m._ir_keep["code"]]


def test_abi_constants(mamba):
    a = mamba.abi
    assert a.MMB_SAMPLER_DGS == 9 and a.MMB_ABI_VERSION == 10
    assert (a.MMB_IR_CATEGORICAL, a.MMB_IR_DISCRETEUNIFORM) == (12, 13)
    assert (a.IR_OP["valv"], a.IR_OP["datav"]) == (7, 8)
    assert a.MMB_DGS_MAX_SUPPORT == 32
    hdr = open(os.path.join(ROOT, "include", "mamba_hip.h")).read()
    for name, val in [("MMB_SAMPLER_DGS", 9), ("MMB_IR_CATEGORICAL", 12), ("MMB_IR_DISCRETEUNIFORM", 13),
                      ("MMB_IR_OP_VALV", 7), ("MMB_IR_OP_DATAV", 8)]:
        assert re.search(rf"\b{name} = {val}\b", hdr), name
    assert re.search(r"#define MMB_ABI_VERSION 10\b", hdr)
    assert re.search(r"#define MMB_DGS_MAX_SUPPORT 32\b", hdr)
    # the fused device opcodes of the new leaves stay inside the opcode byte (engine_ir.cpp ir_fuse)
    assert 64 + 4 * (a.IR_OP["datav"] - 1) + 3 < 256


def test_constructor(mamba):
    a = mamba.abi
    s = mamba.DGS("T")
    assert (s.kind, s.adapt, s.tuning, s.params) == (a.MMB_SAMPLER_DGS, a.MMB_ADAPT_NONE, None, ["T"])
    assert repr(mamba.DGS(["a", "b"])) == "DGS(['a', 'b'])"


@pytest.mark.parametrize("make", ["line", "rats", "logistic"])
def test_non_ir_models_refuse(mamba, make):
    m = mamba.logistic(20, 3, 10.0) if make == "logistic" else getattr(mamba, make)()
    node = {"line": "beta", "rats": "alpha", "logistic": "beta"}[make]
    with pytest.raises(mamba.ArgumentError, match="node-IR"):
        m.setsamplers([mamba.DGS(node)])


def test_discrete_node_needs_dgs(mamba):
    for other in (mamba.AMWG("T", 1.0), mamba.Slice("T", 1.0), mamba.RWM("T", 1.0), mamba.NUTS("T")):
        with pytest.raises(mamba.ArgumentError, match="discrete node T"):
            lowered(mamba, "model2", [other])
    with pytest.raises(mamba.ArgumentError, match="discrete node T"):
        lowered(mamba, "model3", [mamba.AMWG(["T", "mu"], 1.0)])


def test_dgs_on_continuous_node(mamba):
    with pytest.raises(mamba.ArgumentError, match="DGS: node mu"):
        lowered(mamba, "model3", [mamba.DGS("T"), mamba.DGS("mu")])


def test_poisson_stays_observed(mamba):
    ir = mamba.ir
    m = ir.Model(y=ir.Stochastic(1, lambda lam: ir.Poisson(lam), False), lam=ir.Stochastic(lambda: ir.Gamma(1.0, 1.0)))
    m.setsamplers([mamba.DGS("y")])
    with pytest.raises(mamba.ArgumentError, match="DGS: node y"):
        m.init_matrix([{"y": [1, 2], "lam": 1.0}], 1)


def test_support_limit(mamba):
    ir = mamba.ir
    ok = ir.Model(k=ir.Stochastic(1, lambda n: ir.Binomial(n, 0.5))).setinputs({"n": [31.0, 2.0]})
    ok.setsamplers([mamba.DGS("k")]).init_matrix([{"k": [0, 1]}], 1)
    m = ir.Model(k=ir.Stochastic(1, lambda n: ir.Binomial(n, 0.5))).setinputs({"n": [32.0, 2.0]})
    with pytest.raises(mamba.ArgumentError, match="support of 33 values"):
        m.setsamplers([mamba.DGS("k")]).init_matrix([{"k": [0, 1]}], 1)
    m = ir.Model(t=ir.Stochastic(lambda: ir.DiscreteUniform(0, 32)))
    with pytest.raises(mamba.ArgumentError, match="support of 33 values"):
        m.setsamplers([mamba.DGS("t")]).init_matrix([{"t": 1}], 1)
    ir.Model(t=ir.Stochastic(lambda: ir.DiscreteUniform(-3, 28))).setsamplers([mamba.DGS("t")]).init_matrix([{"t": 1}], 1)
    m = ir.Model(t=ir.Stochastic(lambda: ir.Categorical([1.0 / 33] * 33)))
    with pytest.raises(mamba.ArgumentError, match="support of 33 values"):
        m.setsamplers([mamba.DGS("t")]).init_matrix([{"t": 1}], 1)
    # Binomial n must be data
    m = ir.Model(k=ir.Stochastic(lambda lam: ir.Binomial(lam, 0.5)), lam=ir.Stochastic(lambda: ir.Gamma(1.0, 1.0)))
    with pytest.raises(mamba.ArgumentError, match="Binomial n of k must be data"):
        m.setsamplers([mamba.DGS("k"), mamba.Slice("lam", 1.0)]).init_matrix([{"k": 1, "lam": 1.0}], 1)


@pytest.mark.parametrize("p", [[0.5, 0.6], [0.7, -0.2, 0.5], [0.2, float("nan"), 0.8], [0.3, 0.3]])
def test_categorical_needs_a_probability_vector(mamba, p):
    ir = mamba.ir
    m = ir.Model(t=ir.Stochastic(lambda: ir.Categorical(p))).setsamplers([mamba.DGS("t")])
    with pytest.raises(mamba.ArgumentError, match="not a probability vector"):
        m.init_matrix([{"t": 1}], 1)
    md = ir.Model(t=ir.Stochastic(lambda q: ir.Categorical(q))).setinputs({"q": p}).setsamplers([mamba.DGS("t")])
    with pytest.raises(mamba.ArgumentError, match="not a probability vector"):
        md.init_matrix([{"t": 1}], 1)


def test_discrete_uniform_bounds(mamba):
    ir = mamba.ir
    with pytest.raises(mamba.ArgumentError, match="constant integer bounds"):
        ir.DiscreteUniform(1, 2.5)
    with pytest.raises(mamba.ArgumentError, match="a <= b"):
        ir.DiscreteUniform(3, 2)


def test_state_gather_range_and_length(mamba):
    ir = mamba.ir

    def model(K, nT, nmu=3):
        m = ir.Model(y=ir.Stochastic(1, lambda mu, T: ir.Normal(mu[T], 1.0), False),
                     T=ir.Stochastic(1, lambda: ir.Categorical([1.0 / K] * K)))
        m.setinputs({"mu": list(range(nmu))}).setsamplers([mamba.DGS("T")])
        return m, [{"y": [0.0] * 4, "T": [1] * nT}]
    m, ini = model(3, 4)
    m.init_matrix(ini, 1)
    m, ini = model(4, 4)  # support 1..4 against a 3-vector
    with pytest.raises(mamba.ArgumentError, match=r"support 1\.\.4 of T must lie in 1\.\.3"):
        m.init_matrix(ini, 1)
    m, ini = model(3, 5)  # T longer than the expression
    with pytest.raises(mamba.ArgumentError, match="gather index T has length 5, expected 4"):
        m.init_matrix(ini, 1)
    # a Bernoulli index starts at 0
    m = ir.Model(y=ir.Stochastic(1, lambda mu, z: ir.Normal(mu[z], 1.0), False),
                 z=ir.Stochastic(1, lambda: ir.Bernoulli(0.5)))
    m.setinputs({"mu": [0.0, 1.0]}).setsamplers([mamba.DGS("z")])
    with pytest.raises(mamba.ArgumentError, match=r"support 0\.\.1 of z must lie in 1\.\.2"):
        m.init_matrix([{"y": [0.0, 0.0], "z": [0, 1]}], 1)


def test_inits_inside_the_support(mamba):
    m, inputs, inits = dgs_ref.model2(mamba.ir)
    m.setinputs(inputs).setsamplers([mamba.DGS("T")])
    bad = inits(2)
    bad[1]["T"] = [4] + bad[1]["T"][1:]
    with pytest.raises(mamba.ArgumentError, match=r"discrete node T \(chain 2\) is outside its support"):
        m.init_matrix(bad, 2)
    m4, inputs4, inits4 = dgs_ref.model4(mamba.ir)
    m4.setinputs(inputs4).setsamplers([mamba.DGS(["k", "tau"])])
    bad = inits4(1)
    bad[0]["k"] = [4, 0]  # n = [3, 5]
    with pytest.raises(mamba.ArgumentError, match="discrete node k"):
        m4.init_matrix(bad, 1)


def test_key_split_and_block_limit(mamba):
    ir = mamba.ir
    m, _ = lowered(mamba, "model4", [mamba.DGS(["k", "tau"])])
    assert [(s.kind, s.params) for s in m.samplers] == [(9, ["k"]), (9, ["tau"])]
    nodes = {f"z{i}": ir.Stochastic(lambda: ir.Bernoulli(0.5)) for i in range(9)}
    big = ir.Model(**nodes)
    big.setsamplers([mamba.DGS(list(nodes)[:8])])
    with pytest.raises(mamba.ArgumentError, match="need 1..8 sampling blocks"):
        big.setsamplers([mamba.DGS(list(nodes))])
    with pytest.raises(mamba.ArgumentError, match="need 1..8 sampling blocks"):
        big.setsamplers([mamba.DGS(list(nodes)[:5]), mamba.DGS(list(nodes)[5:])])


def test_lowered_model2(mamba):
    a = mamba.abi
    m, V = lowered(mamba, "model2", [mamba.DGS("T")])
    assert V.shape == (4, 40)  # a 40-element DGS block: exempt from the 32-element limit
    I = m.ir()
    y, T = I.nodes[0], I.nodes[1]
    assert (T.family, T.fixed, T.off, T.len, T.lo, T.hi) == (a.MMB_IR_CATEGORICAL, 0, 0, 40, 1.0, 3.0)
    assert list(T.expr) == [-1, -1, -1]
    pool = m._ir_keep["pool"]
    assert list(pool[T.cterm:T.cterm + 3]) == dgs_ref.M2_P
    w = words(m)
    assert w[y.expr[0]] >> 24 == a.IR_OP["datav"] and w[y.expr[0] + 1] == T.off and w[y.expr[0] + 2] == 0
    assert list(pool[(w[y.expr[0]] & 0xffffff):][:3]) == dgs_ref.M2_MU
    B = I.blocks[0]
    assert [B.term[t] for t in range(B.nterms)] == [1, 0]  # the node, then its targets


def test_lowered_model3(mamba):
    a = mamba.abi
    for scheme in ([mamba.DGS("T"), mamba.RWM("mu", 0.3)], [mamba.RWM("mu", 0.3), mamba.DGS("T")]):
        m, V = lowered(mamba, "model3", scheme)
        I = m.ir()
        y, T, mu = I.nodes[0], I.nodes[1], I.nodes[2]
        w = words(m)
        assert w[y.expr[0]] >> 24 == a.IR_OP["valv"] and w[y.expr[0]] & 0xffffff == mu.off == 40
        assert w[y.expr[0] + 1] == T.off == 0
        bd = [s.kind for s in m.samplers].index(a.MMB_SAMPLER_DGS)
        B, Bm = I.blocks[bd], I.blocks[1 - bd]
        assert [B.term[t] for t in range(B.nterms)] == [1, 0]
        assert [Bm.term[t] for t in range(Bm.nterms)] == [2, 0]
        assert m.parents["y"] == {"T", "mu"}


def test_lowered_model4(mamba):
    a = mamba.abi
    m, V = lowered(mamba, "model4", [mamba.DGS(["k", "tau"])])
    I = m.ir()
    r, k, y, tau = (I.nodes[i] for i in range(4))
    assert (k.family, k.fixed, k.lo, k.hi) == (a.MMB_IR_BINOMIAL, 0, 0.0, 5.0)
    assert (tau.family, tau.lo, tau.hi, list(tau.expr), tau.cterm) == (a.MMB_IR_DISCRETEUNIFORM, 1.0, 10.0, [-1] * 3, -1)
    pool = m._ir_keep["pool"]
    w = words(m)
    # n as one data word
    assert w[k.expr[0]] >> 24 == a.IR_OP["data"] and w[k.expr[0] + 1] == 0
    assert list(pool[(w[k.expr[0]] & 0xffffff):][:2]) == dgs_ref.M4_N
    # lchoose(n_i, v), v = 0..5, per element; 0 past n_i
    for i, n in enumerate(dgs_ref.M4_N):
        for v in range(6):
            want = math.lgamma(n + 1) - math.lgamma(v + 1) - math.lgamma(n - v + 1) if v <= n else 0.0
            assert pool[k.cterm + 6 * i + v] == want
    # the observed Poisson keeps its per-element -lgamma(r + 1)
    assert list(pool[r.cterm:r.cterm + 2]) == [-math.lgamma(x + 1) for x in dgs_ref.M4_R]
    assert w[y.expr[0]] >> 24 == a.IR_OP["datav"] and w[y.expr[0] + 1] == tau.off == 2
    assert [[I.blocks[b].term[t] for t in range(I.blocks[b].nterms)] for b in range(2)] == [[1, 0], [3, 2]]


def test_engine_validation_accepts_the_lowered_models(mamba):
    """mmb_ir_jit_prebuild validates the IR like mmb_create_ir and needs no device: the test models pass
    the engine's checks, and the specialised kernel declines them by name."""
    lib = mamba.abi.lib()
    for name, scheme in [("model1", [mamba.DGS("z")]), ("model2", [mamba.DGS("T")]),
                         ("model3", [mamba.RWM("mu", 0.3), mamba.DGS("T")]), ("model4", [mamba.DGS(["k", "tau"])]),
                         ("model5", [mamba.DGS("z")])]:
        m, _ = lowered(mamba, name, scheme)
        spec, I = m.spec(), m.ir()
        buf = C.create_string_buffer(512)
        rc = lib.mmb_ir_jit_prebuild(C.byref(spec), C.byref(I), buf, 512)
        assert rc == -2 and b"DGS" in buf.value, (name, rc, buf.value, lib.mmb_last_error(None))


def test_engine_validation_refuses(mamba):
    lib = mamba.abi.lib()
    buf = C.create_string_buffer(512)

    def rc_of(m):
        spec, I = m.spec(), m.ir()
        return lib.mmb_ir_jit_prebuild(C.byref(spec), C.byref(I), buf, 512), lib.mmb_last_error(None).decode()
    # a support that leaves the indexed table
    m, _ = lowered(mamba, "model2", [mamba.DGS("T")])
    m.ir().nodes[1].hi = 4.0
    rc, msg = rc_of(m)
    assert rc == -1 and ("invalid code" in msg or "constant term" in msg), msg
    # more than 32 support values
    m, _ = lowered(mamba, "model4", [mamba.DGS(["k", "tau"])])
    m.ir().nodes[3].hi = 33.0
    rc, msg = rc_of(m)
    assert rc == -1, msg
    # a discrete node in a block of another kind
    m, _ = lowered(mamba, "model2", [mamba.DGS("T")])
    spec, I = m.spec(), m.ir()
    spec.blocks[0].sampler = mamba.abi.MMB_SAMPLER_SLICE
    assert lib.mmb_ir_jit_prebuild(C.byref(spec), C.byref(I), buf, 512) == -1
    assert "DGS block only" in lib.mmb_last_error(None).decode()


def test_restatement_against_hand_conditionals():
    """Model 1: z_i | rest is Bernoulli with odds 0.3 / 0.7 * N(y_a; m0 + d, 1) N(y_b; m0 + d, 1) /
    (N(y_a; m0, 1) N(y_b; m0, 1)), (a, b) the two observations of group i."""
    spec = dgs_ref.spec1()
    node = spec.blocks[0][1]
    st = {"z": [1.0, 0.0, 1.0]}
    for i in range(3):
        ya, yb = dgs_ref.M1_Y[2 * i], dgs_ref.M1_Y[2 * i + 1]
        m0, d = dgs_ref.M1_M0, dgs_ref.M1_D
        lr = math.log(0.3 / 0.7) + 0.5 * ((ya - m0) ** 2 - (ya - m0 - d) ** 2 + (yb - m0) ** 2 - (yb - m0 - d) ** 2)
        p1 = 1.0 / (1.0 + math.exp(-lr))
        sup, probs = dgs_ref.conditional(node, i, st)
        assert sup == [0, 1] and st["z"] == [1.0, 0.0, 1.0]
        assert probs[1] == pytest.approx(p1, rel=1e-13) and probs[0] == pytest.approx(1.0 - p1, rel=1e-13)
    assert dgs_ref.choose([0.2, 0.5, 0.3], 0.1999) == (0, None)
    assert dgs_ref.choose([0.2, 0.5, 0.3], 0.2) == (1, (0, 1))
    assert dgs_ref.choose([0.2, 0.5, 0.3], 0.7 + 5e-9) == (2, (1, 2))
    assert dgs_ref.choose([0.2, 0.5, 0.3], 0.9999) == (2, None)
    assert dgs_ref.choose([0.0, 0.0], 0.3)[0] == 1  # none exceeds u: the last value
    # psum = 0 and a non-finite psum
    sup, probs = dgs_ref.conditional(dgs_ref.spec5().blocks[0][1], 0, {"z": [0.0]})
    assert probs == [0.5, 0.5]
    inf = dgs_ref.DNode("z", 1, lambda i: [0, 1], lambda i, v, st: 800.0, lambda st: [])
    assert dgs_ref.conditional(inf, 0, {"z": [0.0]})[1] is None


def test_restatement_meets_no_threshold(oracle):
    """The seeds of the GPU replay tests (tests/test_gpu_dgs.py): the restatement alone, run forward from
    the same inits, draws no u within DELTA of a cumulative probability."""
    u = oracle.L.orc_uniform
    import _mamba_path
    ir = _mamba_path.load().ir
    for name, spec, K, iters in [("model1", dgs_ref.spec1(), 8, 200), ("model2", dgs_ref.spec2(), 4, 200),
                                 ("model4", dgs_ref.spec4(), 8, 200), ("model5", dgs_ref.spec5(), 8, 200)]:
        _, _, inits = getattr(dgs_ref, name)(ir)
        hits = 0
        for c, ini in enumerate(inits(K)):
            row = []
            for n in spec.columns:
                row += list(np.atleast_1d(ini[n]).astype(float))
            hits += dgs_ref.forward(u, spec, 11, row, c, iters)[1]
        assert hits == 0, name


def test_observed_binomial_lowering_unchanged(mamba):
    """seeds (an observed Binomial node): code, pool, constants, node and block tables byte for byte what
    the lowering produced before discrete nodes could be sampled (digest recorded from that version)."""
    ir = mamba.ir
    m = ir.seeds_model().setinputs(ir.SEEDS)
    m.setsamplers([mamba.AMWG(["alpha0", "alpha1", "alpha2", "alpha12"], 0.1), mamba.AMWG("b", 0.1),
                   mamba.Slice("s2", 1.0)])
    m.init_matrix(ir.seeds_inits(), 2)
    I, k = m.ir(), m._ir_keep
    h = hashlib.sha256()
    for part in (np.asarray(k["code"]).tobytes(), np.asarray(k["pool"]).tobytes(), np.asarray(k["consts"]).tobytes(),
                 bytes(k["nodes"]), np.asarray(k["mon"]).tobytes()):
        h.update(part)
    for b in range(len(m.samplers)):
        h.update(bytes(I.blocks[b]))
    assert h.hexdigest() == "6cbdb1225256a958608df2fee708c94b2d2e70d5289ac4a22e9cf1bba35a5d7e"
