"""BMG, BMC3 and BIA (src/samplers/bmg.jl, bmc3.jl, bia.jl) on the CPU: the constants, the constructors and every
refusal of the host and of the engine's validation, the lowered block specs, the tune row's length, the
restatement (tests/binary_ref.py) against hand-computed conditionals, the index draw's frequencies, and the
restatement alone on the seeds of the GPU replay tests."""
import ctypes as C
import itertools
import math
import os
import re

import numpy as np
import pytest

import binary_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 11  # the GPU tests' seed (tests/test_gpu_binary.py)


def lowered(mamba, D, scheme, K=4, prior="bernoulli", mixed=False):
    m, inputs, inits = br.model(mamba.ir, D, prior, mixed)
    m.setinputs(inputs).setsamplers(scheme)
    return m, m.init_matrix(inits(K), K)


def test_abi_constants(mamba):
    a = mamba.abi
    assert (a.MMB_SAMPLER_BMG, a.MMB_SAMPLER_BMC3, a.MMB_SAMPLER_BIA) == (11, 12, 13)
    assert a.MMB_ABI_VERSION == 10 and a.MMB_SUB_BINARY == 7 == br.SUB_BINARY
    assert (a.MMB_BINARY_K_INT, a.MMB_BINARY_K_LISTS, a.MMB_BINARY_MAX_LISTS, a.MMB_BINARY_MAX) == (0, 1, 64, 32)
    hdr = open(os.path.join(ROOT, "include", "mamba_hip.h")).read()
    for name, val in [("MMB_SAMPLER_BMG", 11), ("MMB_SAMPLER_BMC3", 12), ("MMB_SAMPLER_BIA", 13),
                      ("MMB_BINARY_K_INT", 0), ("MMB_BINARY_K_LISTS", 1)]:
        assert re.search(rf"\b{name} = {val}\b", hdr), name
    assert re.search(r"#define MMB_ABI_VERSION 10\b", hdr)
    assert re.search(r"#define MMB_BINARY_MAX_LISTS 64\b", hdr) and re.search(r"#define MMB_BINARY_MAX 32\b", hdr)
    mh = open(os.path.join(ROOT, "mamba.jl_amd", "csrc", "mmb_math.h")).read()
    assert re.search(r"#define MMB_SUB_BINARY 7u\b", mh)
    jl = open(os.path.join(ROOT, "julia", "MambaHIP.jl")).read()
    assert "MMB_SAMPLER_BMG, MMB_SAMPLER_BMC3, MMB_SAMPLER_BIA = Int32(11), Int32(12), Int32(13)" in jl


def test_constructors(mamba):
    a = mamba.abi
    s = mamba.BMG("gamma")
    assert (s.kind, s.adapt, s.tuning, s.params, s.k, s.form, s.nsteps) == \
        (a.MMB_SAMPLER_BMG, a.MMB_ADAPT_NONE, None, ["gamma"], 1, a.MMB_BINARY_K_INT, 1)
    s = mamba.BMC3(["gamma"], k=[[1], [2, 3]])
    assert (s.kind, s.k, s.form) == (a.MMB_SAMPLER_BMC3, [[1], [2, 3]], a.MMB_BINARY_K_LISTS)
    s = mamba.BIA("gamma")
    assert (s.kind, s.beta, s.target, s.bia) == (a.MMB_SAMPLER_BIA, 0.55, 0.45, (None, None, None))
    assert repr(mamba.BMG("g", k=2)) == "BMG(['g'])" and repr(mamba.BMC3("g")) == "BMC3(['g'])"
    assert repr(mamba.BIA("g")) == "BIA(['g'])"
    for bad in (0, -1, [], [[]], [[0]], [[1.5]], "ab", [[1]] * 65):
        with pytest.raises(mamba.ArgumentError):
            mamba.BMG("g", k=bad)
    mamba.BMC3("g", k=[[1]] * 64)


@pytest.mark.parametrize("make", ["line", "rats", "logistic"])
@pytest.mark.parametrize("smp", ["BMG", "BMC3", "BIA"])
def test_non_ir_models_refuse(mamba, make, smp):
    m = mamba.logistic(20, 3, 10.0) if make == "logistic" else getattr(mamba, make)()
    node = {"line": "beta", "rats": "alpha", "logistic": "beta"}[make]
    with pytest.raises(mamba.ArgumentError, match="node-IR"):
        m.setsamplers([getattr(mamba, smp)(node)])


@pytest.mark.parametrize("smp", ["BMG", "BMC3", "BIA"])
def test_key_list_refused(mamba, smp):
    with pytest.raises(mamba.ArgumentError, match="one joint step"):
        getattr(mamba, smp)(["a", "b"])


@pytest.mark.parametrize("smp", ["BMG", "BMC3", "BIA"])
def test_family_refusals(mamba, smp):
    ir = mamba.ir
    S = getattr(mamba, smp)
    # a continuous node
    with pytest.raises(mamba.ArgumentError, match=f"{smp}: node beta is not a Bernoulli"):
        lowered(mamba, br.MIX, [S("beta"), mamba.DGS("gamma"), mamba.Slice("s2", 1.0)], mixed=True)
    # non-binary discrete nodes, by name
    for dist, init in ((lambda: ir.DiscreteUniform(0, 2), 1), (lambda: ir.DiscreteUniform(1, 2), 1),
                       (lambda: ir.Categorical([0.5, 0.5]), 1)):
        m = ir.Model(t=ir.Stochastic(1, dist)).setsamplers([S("t")])
        with pytest.raises(mamba.ArgumentError, match=f"{smp}: node t is not a Bernoulli"):
            m.init_matrix([{"t": [init, init]}], 1)
    m = ir.Model(t=ir.Stochastic(1, lambda n: ir.Binomial(n, 0.5))).setinputs({"n": [1.0, 1.0]}).setsamplers([S("t")])
    with pytest.raises(mamba.ArgumentError, match=f"{smp}: node t is not a Bernoulli"):
        m.init_matrix([{"t": [0, 1]}], 1)
    # more than 32 elements
    m = ir.Model(t=ir.Stochastic(1, lambda: ir.Bernoulli(0.5))).setsamplers([S("t")])
    with pytest.raises(mamba.ArgumentError, match="at most 32 elements"):
        m.init_matrix([{"t": [0] * 33}], 1)
    # the other kinds still refuse a discrete node in their own words
    with pytest.raises(mamba.ArgumentError, match="discrete node gamma"):
        lowered(mamba, br.S3, [mamba.Slice("gamma", 1.0)])


def test_k_refusals(mamba):
    for S in (mamba.BMG, mamba.BMC3):
        lowered(mamba, br.S3, [S("gamma", k=3)])
        with pytest.raises(mamba.ArgumentError, match="k exceeds variate length 3"):
            lowered(mamba, br.S3, [S("gamma", k=4)])
        lowered(mamba, br.S3, [S("gamma", k=[[1, 3], [2]])])
        with pytest.raises(mamba.ArgumentError, match="indices in k exceed variate length 3"):
            lowered(mamba, br.S3, [S("gamma", k=[[1], [2, 4]])])
        with pytest.raises(mamba.ArgumentError, match="indices in k start at 1"):
            S("gamma", k=[[0, 1]])
        with pytest.raises(mamba.ArgumentError, match="1..64 index lists"):
            S("gamma", k=[[1]] * 65)


def test_bia_validation(mamba):
    """bia.jl:36-50, in its order; the defaults A = D = 1 / n fail it for n = 1 (1 / 1 is not below 1 - epsilon)."""
    ok = lowered(mamba, br.S3, [mamba.BIA("gamma")])[0].samplers[0]
    assert ok.epsilon == 0.01 / 3 and list(ok.tuning) == [1.0 / 3] * 6
    for kw, msg in [(dict(epsilon=0.5), r"epsilon is not in \(0, 0.5\)"), (dict(epsilon=0.0), "epsilon is not in"),
                    (dict(A=[0.2, 0.2]), "A must contain 3 probabilities"),
                    (dict(A=[0.2, 0.2, 0.001]), "A must contain 3 probabilities"),
                    (dict(D=[0.2, 0.999, 0.2]), "D must contain 3 probabilities"),
                    (dict(decay=0.5), r"decay is not in \(0.5, 1\]"), (dict(decay=1.01), "decay is not in"),
                    (dict(target=0.0), r"target is not in \(0, 1\)"), (dict(target=1.0), "target is not in")]:
        with pytest.raises(mamba.ArgumentError, match=msg):
            lowered(mamba, br.S3, [mamba.BIA("gamma", **kw)])
    with pytest.raises(mamba.ArgumentError, match="A must contain 1 probabilities"):
        lowered(mamba, br.S1, [mamba.BIA("gamma")])
    lowered(mamba, br.S1, [mamba.BIA("gamma", A=[0.5], D=[0.5])])


@pytest.mark.parametrize("smp", ["BMG", "BMC3", "BIA"])
def test_inits_are_binary(mamba, smp):
    for prior in ("bernoulli", "uniform"):
        m, inputs, inits = br.model(mamba.ir, br.S3, prior)
        m.setinputs(inputs).setsamplers([getattr(mamba, smp)("gamma")])
        for v in (2.0, 0.5, -1.0):
            bad = inits(2)
            bad[1]["gamma"] = [v, 0.0, 1.0]
            with pytest.raises(mamba.ArgumentError, match=r"discrete node gamma \(chain 2\) is outside its support"):
                m.init_matrix(bad, 2)


def test_lowered_block_specs(mamba):
    a = mamba.abi
    m, V = lowered(mamba, br.S6, [mamba.BMG("gamma", k=3)])
    assert V.shape == (4, 6) and set(np.unique(V)) <= {0.0, 1.0}
    b = m.spec().blocks[0]
    assert (b.sampler, b.nnodes, b.dim, b.form, b.nsteps, b.ntuning) == (11, 1, 6, a.MMB_BINARY_K_INT, 3, 0)
    I = m.ir()
    y, g = I.nodes[0], I.nodes[1]
    assert (g.family, g.fixed, g.len, g.lo, g.hi) == (a.MMB_IR_BERNOULLI, 0, 6, 0.0, 1.0)
    assert [I.blocks[0].term[t] for t in range(I.blocks[0].nterms)] == [1, 0]  # the node, then its target
    m, _ = lowered(mamba, br.S6, [mamba.BMC3("gamma", k=[[1], [2, 3], [4, 5, 6], [6, 1, 1]])])
    sp = m.spec()
    b = sp.blocks[0]
    assert (b.sampler, b.form, b.ntuning) == (12, a.MMB_BINARY_K_LISTS, 4)
    assert [b.tuning[i] for i in range(4)] == [1.0, 6.0, 56.0, 33.0]
    m, _ = lowered(mamba, br.S32, [mamba.BMG("gamma", k=[[32], [1, 32]])], prior="uniform")
    sp = m.spec()
    assert [sp.blocks[0].tuning[i] for i in range(2)] == [2.0 ** 31, 2.0 ** 31 + 1.0]
    assert (m.ir().nodes[1].family, m.ir().nodes[1].hi) == (a.MMB_IR_DISCRETEUNIFORM, 1.0)
    m, _ = lowered(mamba, br.S3, [mamba.BIA("gamma", A=[0.2, 0.3, 0.4], D=[0.5, 0.6, 0.7], epsilon=0.01, decay=0.6,
                                            target=0.3)])
    sp = m.spec()
    b = sp.blocks[0]
    assert (b.sampler, b.epsilon, b.beta, b.target, b.ntuning) == (13, 0.01, 0.6, 0.3, 6)
    assert [b.tuning[i] for i in range(6)] == [0.2, 0.3, 0.4, 0.5, 0.6, 0.7]


SCHEMES = [("S6", "BMG", dict(k=3)), ("S6", "BMC3", dict(k=[[1], [2, 3], [4, 5, 6]])), ("S32", "BMG", dict(k=5)),
           ("S1", "BMG", {}), ("S6", "BIA", {}), ("S32", "BIA", {}), ("EDGE", "BMG", dict(k=3))]


def test_engine_validation_accepts_the_lowered_models(mamba):
    """mmb_ir_jit_prebuild validates the IR and the block specs like mmb_create_ir and needs no device: the test
    models pass, and the specialised kernel declines them naming the sampler."""
    lib = mamba.abi.lib()
    for dn, smp, kw in SCHEMES:
        m, _ = lowered(mamba, getattr(br, dn), [getattr(mamba, smp)("gamma", **kw)], prior=br.prior_of(dn))
        spec, I = m.spec(), m.ir()
        buf = C.create_string_buffer(512)
        rc = lib.mmb_ir_jit_prebuild(C.byref(spec), C.byref(I), buf, 512)
        assert rc == -2 and smp.encode() in buf.value, (dn, smp, rc, buf.value, lib.mmb_last_error(None))
    for first in (True, False):
        bl = [mamba.BMG("gamma", k=2)]
        ot = [mamba.RWM("beta", 0.3), mamba.Slice("s2", 1.0, transform=True)]
        m, _ = lowered(mamba, br.MIX, bl + ot if first else ot + bl, mixed=True)
        spec, I = m.spec(), m.ir()
        buf = C.create_string_buffer(512)
        assert lib.mmb_ir_jit_prebuild(C.byref(spec), C.byref(I), buf, 512) == -2 and b"BMG" in buf.value


def test_engine_validation_refuses(mamba):
    lib, a = mamba.abi.lib(), mamba.abi
    buf = C.create_string_buffer(512)

    def rc_of(spec, I):
        return lib.mmb_ir_jit_prebuild(C.byref(spec), C.byref(I), buf, 512), lib.mmb_last_error(None).decode()
    # a Binomial node patched into a BMG block: refused by name
    ir = mamba.ir
    m = ir.Model(t=ir.Stochastic(1, lambda n: ir.Binomial(n, 0.5))).setinputs({"n": [1.0, 1.0]})
    m.setsamplers([mamba.DGS("t")]).init_matrix([{"t": [0, 1]}], 1)
    spec, I = m.spec(), m.ir()
    spec.blocks[0].sampler, spec.blocks[0].nsteps = a.MMB_SAMPLER_BMG, 1
    rc, msg = rc_of(spec, I)
    assert rc == -1 and "BMG" in msg and "not binary" in msg, msg
    # a binary node in a Slice block: the engine's old words
    m, _ = lowered(mamba, br.S3, [mamba.BMG("gamma")])
    spec, I = m.spec(), m.ir()
    spec.blocks[0].sampler = a.MMB_SAMPLER_SLICE
    rc, msg = rc_of(spec, I)
    assert rc == -1 and "DGS block only" in msg, msg
    # the block spec's own fields: mmb_create_ir checks them after the IR, before it touches a device

    def rc_of(spec, I):  # noqa: F811
        h = C.c_void_p()
        rc = lib.mmb_create_ir(C.byref(spec), C.byref(I), 0, C.byref(h))
        assert not h.value
        return rc, lib.mmb_last_error(None).decode()
    for patch, want in [(lambda b: setattr(b, "nsteps", 4), "k exceeds variate length 3"),
                        (lambda b: setattr(b, "nsteps", 0), "k exceeds variate length 3"),
                        (lambda b: setattr(b, "form", 2), "unknown form")]:
        m, _ = lowered(mamba, br.S3, [mamba.BMG("gamma")])
        spec, I = m.spec(), m.ir()
        patch(spec.blocks[0])
        rc, msg = rc_of(spec, I)
        assert rc == -1 and want in msg, msg
    m, _ = lowered(mamba, br.S3, [mamba.BMC3("gamma", k=[[1], [3]])])
    spec, I = m.spec(), m.ir()
    spec.blocks[0].tuning[1] = 8.0  # element 4 of 3
    rc, msg = rc_of(spec, I)
    assert rc == -1 and "indices in k exceed variate length 3" in msg, msg
    for field, val, want in [("epsilon", 0.5, "epsilon is not in"), ("beta", 0.5, "decay is not in"),
                             ("target", 1.0, "target is not in"), ("ntuning", 5, "A and D must contain 3")]:
        m, _ = lowered(mamba, br.S3, [mamba.BIA("gamma")])
        spec, I = m.spec(), m.ir()
        setattr(spec.blocks[0], field, val)
        rc, msg = rc_of(spec, I)
        assert rc == -1 and want in msg, msg
    m, _ = lowered(mamba, br.S3, [mamba.BIA("gamma")])
    spec, I = m.spec(), m.ir()
    spec.blocks[0].tuning[4] = 0.999
    rc, msg = rc_of(spec, I)
    assert rc == -1 and "D must contain 3 probabilities" in msg, msg


def test_tune_len(mamba):
    """The canonical tune row: BMG and BMC3 none, BIA [iter, A[d], D[d]] (mmb_tune_len needs an engine, and an
    engine a device: the length is read off the source's table and the Python mirror of the row)."""
    src = open(os.path.join(ROOT, "mamba.jl_amd", "csrc", "engine_tune.cpp")).read()
    assert re.search(r"case MMB_SAMPLER_BIA: return 1 \+ 2 \* d;", src)
    assert re.search(r"case MMB_SAMPLER_BMG: return 0;", src) and re.search(r"case MMB_SAMPLER_BMC3: return 0;", src)
    node = br.spec(br.S6, "bia").blocks[0][1]
    st = {"gamma": [0.0] * 6}
    u = lambda j: 0.9  # noqa: E731
    out = br.bia_step(node, st, [0.0] + [1.0 / 6] * 12, u, u, br.Dec())
    assert len(out[2]) == 1 + 2 * 6 and out[2][0] == 1.0


def test_restatement_against_hand_conditionals():
    """S3: gamma_i | rest has odds exp(sum_obs ((y - mu0)^2 - (y - mu1)^2) / 2) (the priors cancel), which is BMG's p_i;
    BMC3's ratio is the same odds; BIA's A', D' against the formulas of bia.jl:101-111 by hand."""
    D = br.S3
    node = br.spec(D, "bmg", k=3).blocks[0][1]
    g = [1.0, 0.0, 1.0]
    st = {"gamma": list(g)}

    def mu(gv, o):
        return sum(D.X[j][o] * D.b0[j] * gv[j] for j in range(3))
    probs = [0.5] * 3
    br._pbernoulli(node, st, g, node.logf(st, g), [0, 1, 2], probs)
    for i in range(3):
        g1, g0 = list(g), list(g)
        g1[i], g0[i] = 1.0, 0.0
        lr = sum(0.5 * ((D.y[o] - mu(g0, o)) ** 2 - (D.y[o] - mu(g1, o)) ** 2) for o in range(br.NOBS))
        assert probs[i] == pytest.approx(1.0 / (1.0 + math.exp(-lr)), rel=1e-12)
    assert st["gamma"] == g and node.evals == 4  # logf(x) once, one more per element
    # BMC3, k = 3 flips everything: accept iff u < exp(logf(1 - g) - logf(g))
    n3 = br.spec(D, "bmc3", k=3).blocks[0][1]
    flip = [1.0 - v for v in g]
    ratio = math.exp(n3.logf(st, flip) - n3.logf(st, g))
    for u0, acc in ((ratio * 0.99, True), (min(ratio * 1.01, 0.999999), ratio * 1.01 > 1.0)):
        if u0 < 1.0:
            out = br.bmc3_step(n3, st, lambda j: 0.3, lambda j, u0=u0: u0, br.Dec())
            assert out == ((flip if acc else g), acc)
    # the 2k + 2 evaluations of a BMG update
    node.evals = 0
    br.bmg_step(node, st, lambda j: 0.3, lambda j: 0.4, br.Dec())
    assert node.evals == 2 * 3 + 2
    n3.evals = 0
    br.bmc3_step(n3, st, lambda j: 0.3, lambda j: 0.4, br.Dec())
    assert n3.evals == 2
    # BIA by hand: nothing proposed (u = 0.99): alpha = 1, A and D only pass through the log / exp round trip
    nb = br.spec(D, "bia").blocks[0][1]
    row = [4.0, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7]
    v, acc, new = br.bia_step(nb, st, row, lambda j: 0.99, lambda j: 0.5, br.Dec())
    assert v == g and acc and new[0] == 5.0 and nb.evals == 2
    assert new[1:] == pytest.approx(row[1:], rel=1e-14)
    # element 2 (a 0) added with u < A_2: alpha = min(1, odds * D_2 / A_2), A_2 moves by 5^-0.55 (alpha - 0.45) on the
    # logit scale of (A - eps) / (1 - A - eps)
    ub = lambda j: 0.25 if j == 1 else 0.99  # noqa: E731
    v, acc, new = br.bia_step(nb, st, row, ub, lambda j: 0.0, br.Dec())
    x = [1.0, 1.0, 1.0]
    alpha = min(1.0, math.exp(nb.logf(st, x) - nb.logf(st, g)) * 0.6 / 0.3)
    eps = 0.01 / 3
    c = math.log((0.3 - eps) / (1 - 0.3 - eps)) + 5.0 ** -0.55 * (alpha - 0.45)
    assert v == x and acc
    assert new[2] == pytest.approx((math.exp(c) * (1 - eps) + eps) / (1 + math.exp(c)), rel=1e-13)
    assert new[1] == pytest.approx(0.2, rel=1e-14) and new[5] == pytest.approx(0.6, rel=1e-14)
    # near comparisons branch: explore returns both outcomes
    outs = br.explore(lambda d: br.bmc3_step(n3, st, lambda j: 0.3, lambda j: ratio + 5e-9 if ratio < 1 else 0.5, d))
    assert len(outs) == (2 if ratio < 1 else 1)


def test_edge_model_takes_the_half_branch():
    """EDGE: over all 8 states, some p_i rounds to 1 (difference above 40) and some to 0 (below -800, exp overflows),
    and no difference lies near either rounding boundary (36.7 and 709.8), where the device's own rounding could
    decide the 0 < p < 1 test the other way."""
    node = br.spec(br.EDGE, "bmg", k=3).blocks[0][1]
    big = huge = 0
    for g in itertools.product([0.0, 1.0], repeat=3):
        st = {"gamma": list(g)}
        for i in range(3):
            g1, g0 = list(g), list(g)
            g1[i], g0[i] = 1.0, 0.0
            d = node.logf(st, g1) - node.logf(st, g0)
            assert not 34.0 < d < 40.0 and not 650.0 < -d < 800.0 and not 650.0 < d < 800.0, (g, i, d)
            big += d > 40.0
            huge += d < -800.0
    assert big > 0 and huge > 0
    node.halves = 0
    br.bmg_step(node, {"gamma": [0.0, 1.0, 0.0]}, lambda j: 0.3, lambda j: 0.4, br.Dec())
    assert node.halves > 0


def test_index_draw_frequencies(oracle):
    """Each element is in the index set with frequency k / n over 20000 streams, within 5 standard errors; the list
    form picks each list with frequency 1 / m."""
    u = oracle.L.orc_uniform
    N = 20000
    for n, k in ((6, 1), (6, 3), (32, 5), (5, 5)):
        cnt = np.zeros(n)
        for c in range(N):
            idx = br.index_set(lambda j: u(SEED, c, 1, 0, br.SUB_BINARY, j), n, k)
            assert len(idx) == k == len(set(idx)) and min(idx) >= 0 and max(idx) < n
            cnt[idx] += 1
        p = k / n
        assert np.all(np.abs(cnt / N - p) <= 5.0 * math.sqrt(p * (1.0 - p) / N) + 1e-15), (n, k, cnt / N)
    lists = [[1], [2, 3], [4, 5, 6]]
    cnt = np.zeros(3)
    for c in range(N):
        idx = br.index_set(lambda j: u(SEED, c, 1, 0, br.SUB_BINARY, j), 6, lists)
        cnt[[[0], [1, 2], [3, 4, 5]].index(idx)] += 1
    assert np.all(np.abs(cnt / N - 1 / 3) <= 5.0 * math.sqrt(2 / 9 / N))


def test_restatement_meets_no_threshold(oracle):
    """The seed and chain counts of the GPU replay tests: the restatement alone, run forward from the same inits,
    meets no comparison within DELTA of its threshold (about 1e5 comparisons at 2e-8 each)."""
    u = oracle.L.orc_uniform
    import _mamba_path
    ir = _mamba_path.load().ir
    for dn, kind, k, K, iters in br.REPLAY_CASES + br.BIA_CASES + [br.EDGE_CASE]:
        D = getattr(br, dn)
        _, _, inits = br.model(ir, D)
        sp = br.spec(D, kind, k)
        hits = 0
        for c, ini in enumerate(inits(K)):
            hits += br.forward(u, sp, SEED, [float(v) for v in ini["gamma"]], c, iters)[1]
        assert hits == 0, (D.n, kind, k)
