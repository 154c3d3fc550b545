"""ABC (src/samplers/abc.jl:23-147) on the host: the constructor's validation, the lowering of a model to its data
nodes, T and the tune row, the ABI mirror, csrc/abc.h's kernel densities, and the Python restatement
(tests/abc_ref.py) alone on a model whose ABC target is the exact posterior."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import abc_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ 1. the ABI mirror
def test_abi_constants(mamba):
    a = mamba.abi
    assert a.MMB_SAMPLER_ABC == 15 and a.MMB_ABI_VERSION == 10
    assert (a.MMB_ABC_MAX_DRAW, a.MMB_ABC_MAX_NSIM, a.MMB_ABC_MAX_T, a.MMB_ABC_MAX_DATA, a.MMB_ABC_MAX_SUMMARY) == \
        (1024, 8, 32, 16, 8) == (ar.MAX_DRAW, ar.MAX_NSIM, 32, 16, 8)
    assert (a.MMB_SUB_ABC_N, a.MMB_SUB_ABC_U) == (ar.SUB_ABC_N, ar.SUB_ABC_U) == (8, 9)
    assert [a.MMB_ABC_IDENTITY, a.MMB_ABC_SUM, a.MMB_ABC_MEAN, a.MMB_ABC_VAR, a.MMB_ABC_STD, a.MMB_ABC_MINIMUM,
            a.MMB_ABC_MAXIMUM] == list(range(7))
    hdr = open(os.path.join(ROOT, "include", "mamba_hip.h")).read()
    assert re.search(r"\bMMB_SAMPLER_ABC = 15\b", hdr) and re.search(r"#define MMB_ABI_VERSION 10\b", hdr)
    for name, val in (("MAX_DRAW", 1024), ("MAX_NSIM", 8), ("MAX_T", 32), ("MAX_DATA", 16), ("MAX_SUMMARY", 8)):
        assert int(re.search(rf"#define MMB_ABC_{name} (\d+)", hdr).group(1)) == val
    assert re.search(r"MMB_ABC_IDENTITY = 0, MMB_ABC_SUM = 1, MMB_ABC_MEAN = 2, MMB_ABC_VAR = 3, MMB_ABC_STD = 4, "
                     r"MMB_ABC_MINIMUM = 5,\s+MMB_ABC_MAXIMUM = 6", hdr)
    mh = open(os.path.join(ROOT, "mamba.jl_amd", "csrc", "mmb_math.h")).read()
    assert re.search(r"#define MMB_SUB_ABC_N 8u\b", mh) and re.search(r"#define MMB_SUB_ABC_U 9u\b", mh)
    assert "MMB_SAMPLER_ABC = Int32(15)" in open(os.path.join(ROOT, "julia", "MambaHIP.jl")).read()
    # the simulation blocks fit the 28 bits a block index has (the tag is block * 16 + substream, 32 bits)
    assert ar.abc_block(7, ar.MAX_DRAW, ar.MAX_NSIM - 1, 16) < 1 << 28


# ------------------------------------------------------------------ 2. the constructor
def test_constructor_defaults_and_packing(mamba):
    a = mamba.abi
    s = mamba.ABC("beta", [0.5, 0.25], "identity", 0.5)
    assert (s.kind, s.name, repr(s), s.params, s.adapt, s.transform) == \
        (15, "ABC", "ABC(['beta'])", ["beta"], a.MMB_ADAPT_NONE, 1)
    # abc.jl:23-29: kernel = SymUniform, proposal = Normal, maxdraw = nsim = 1, decay = 1.0, randeps = false
    assert (s.form, s.batchsize, s.nsteps, s.beta, s.epsilon) == (a.MMB_RWM_SYMUNIFORM << 8, 1, 1, 1.0, 0.5)
    assert (s.maxdraw, s.nsim, s.decay, s.randeps, s.abc_codes) == (1, 1, 1.0, False, [0])
    s = mamba.ABC(["a", "b"], 2, ("mean", "STD"), 0.1, kernel="epanechnikov", proposal=mamba.Cosine, maxdraw=100, nsim=3,
                  decay=0.25, randeps=True)
    assert s.form == a.MMB_RWM_COSINE | a.MMB_RWM_EPANECHNIKOV << 8 | 1 << 16
    assert (s.batchsize, s.nsteps, s.beta, s.epsilon, s.abc_codes) == (100, 3, 0.25, 0.1, [2, 4])
    np.testing.assert_array_equal(s.spec_tuning(3), [2.0, 2.0, 2.0, 2.0, 4.0])
    with pytest.raises(mamba.ArgumentError, match="once its model has its initial values"):
        s.tune_len(3)


def test_constructor_validation(mamba):
    E, A = mamba.ArgumentError, mamba.ABC
    for decay in (-0.1, 1.5, math.nan, "x"):
        with pytest.raises(E, match=r"decay is not in \[0, 1\]"):
            A("p", 1.0, "sum", 0.5, decay=decay)
    for eps in (0.0, -1.0, math.inf, math.nan, "e"):
        with pytest.raises(E, match="epsilon is not finite and > 0"):
            A("p", 1.0, "sum", eps)
    for md in (0, 1025, 1.5, True):
        with pytest.raises(E, match="maxdraw is not an integer in 1..1024"):
            A("p", 1.0, "sum", 0.5, maxdraw=md)
    for ns in (0, 9, 2.0):
        with pytest.raises(E, match="nsim is not an integer in 1..8"):
            A("p", 1.0, "sum", 0.5, nsim=ns)
    with pytest.raises(E, match="randeps is True or False"):
        A("p", 1.0, "sum", 0.5, randeps=1)
    with pytest.raises(E, match="unsupported summary median"):
        A("p", 1.0, ("mean", "median"), 0.5)
    with pytest.raises(E, match="unsupported summary"):
        A("p", 1.0, (lambda x: x,), 0.5)
    with pytest.raises(E, match="identity summary may only stand alone"):
        A("p", 1.0, ("identity", "mean"), 0.5)
    with pytest.raises(E, match="summary lists 1..8"):
        A("p", 1.0, (), 0.5)
    with pytest.raises(E, match="unsupported kernel Gaussian"):
        A("p", 1.0, "sum", 0.5, kernel="Gaussian")
    with pytest.raises(E, match="unsupported proposal Laplace"):
        A("p", 1.0, "sum", 0.5, proposal="Laplace")
    with pytest.raises(E, match="dist: only None"):
        A("p", 1.0, "sum", 0.5, dist=lambda a, b: 0.0)
    for sc in (-1.0, [1.0, math.inf], math.nan, []):
        with pytest.raises(E, match="scale must be a finite non-negative"):
            A("p", sc, "sum", 0.5)
    for nm in ar.KERNELS:  # the seven names, in any letter case, for both
        A("p", 0.0, "sum", 0.5, kernel=nm.upper(), proposal=nm.lower())


@pytest.mark.parametrize("make", ["line", "rats", "logistic"])
def test_non_ir_models_refuse(mamba, make):
    m = mamba.logistic(20, 3, 10.0) if make == "logistic" else getattr(mamba, make)()
    node = {"line": "beta", "rats": "alpha", "logistic": "beta"}[make]
    with pytest.raises(mamba.ArgumentError, match="node-IR"):
        m.setsamplers([mamba.ABC(node, 1.0, "sum", 0.5)])


# ------------------------------------------------------------------ 3. lowering: data nodes, T, tune_len
def test_lowering_data_nodes_T_and_tune_len(mamba):
    a = mamba.abi
    m, V, data, tw, tb = ar.line_abc(mamba, 3)
    s0, s1 = m.samplers
    assert (s0.abc_data, s0.abc_T, s1.abc_data, s1.abc_T) == (["y"], 5, ["y"], 2)
    assert [s.tune_len(m.block_dim(s)) for s in m.samplers] == [1 + 3 * 7, 1 + 3 * 4]
    sp = m.spec()
    b0, b1 = sp.blocks[0], sp.blocks[1]
    assert (b0.sampler, b0.dim, b0.form, b0.batchsize, b0.nsteps, b0.beta, b0.epsilon, b0.transform, b0.ntuning) == \
        (15, 2, a.MMB_RWM_NORMAL << 8, 4, 3, 1.0, 0.5, 1, 3)
    assert [b0.tuning[i] for i in range(3)] == [0.5, 0.25, 0.0]
    assert (b1.form, b1.ntuning, [b1.tuning[i] for i in range(3)]) == (a.MMB_RWM_EPANECHNIKOV << 8, 3, [0.5, 2.0, 4.0])
    I = m.ir()
    assert [(I.blocks[0].term[t], I.blocks[0].trans[t]) for t in range(I.blocks[0].nterms)] == [(1, 1), (0, 0)]
    # five concatenated nodes, in the block's term order; a hierarchical data node that another block samples
    m, *_ = ar.families(mamba, 2)
    assert (m.samplers[0].abc_data, m.samplers[0].abc_T) == (["yb", "yn", "yp", "ye", "yu"], 15)
    m, *_ = ar.hierarchical(mamba, 2)
    assert (m.samplers[0].abc_data, m.samplers[0].abc_T, m.samplers[0].tune_len(1)) == (["theta"], 2, 1 + 2 * 4)
    m, *_ = ar.wide(mamba, 2)
    assert (m.samplers[0].abc_T, m.samplers[0].tune_len(2)) == (6, 1 + 2 * 8)
    m, *_ = ar.caps(mamba, 2)
    assert (m.samplers[0].abc_T, m.samplers[0].tune_len(1)) == (32, 1 + 8 * 34)
    src = open(os.path.join(ROOT, "mamba.jl_amd", "csrc", "engine_tune.cpp")).read()
    assert re.search(r"case MMB_SAMPLER_ABC: return 1 \+ nsim \* \(nstat \+ 2\);", src)


def _one(mamba, ydist, summary="identity", n=3, prior=None, inputs=None, y=None, **kw):
    ir = mamba.ir
    m = ir.Model(y=ir.Stochastic(1, ydist, False),
                 p=ir.Stochastic(prior or (lambda: ir.Gamma(2.0, 1.0))))
    m.setinputs(inputs or {}).setsamplers([mamba.ABC("p", 1.0, summary, 0.5, **kw)])
    return m, [{"y": [1.0] * n if y is None else y, "p": 0.5}]


def test_lowering_refusals(mamba):
    ir, E = mamba.ir, mamba.ArgumentError
    # no data node: the block's node has no stochastic target
    m = ir.Model(p=ir.Stochastic(lambda: ir.Gamma(2.0, 1.0))).setsamplers([mamba.ABC("p", 1.0, "sum", 0.5)])
    with pytest.raises(E, match="needs at least one data node"):
        m.init_matrix([{"p": 0.5}], 1)
    # the families whose variates need a rejection loop, and the categorical ones, by name
    for dist, name in ((lambda p: ir.Gamma(2.0, p), "Gamma"), (lambda p: ir.InverseGamma(2.0, p), "InverseGamma"),
                       (lambda p: ir.Beta(2.0, p), "Beta")):
        m, inits = _one(mamba, dist, y=[0.5, 0.5, 0.5])
        with pytest.raises(E, match=f"cannot simulate data node y: {name} data nodes"):
            m.init_matrix(inits, 1)
    # T over 32, and var / std of a one-element node
    m, inits = _one(mamba, lambda p: ir.Exponential(p), n=33)
    with pytest.raises(E, match="total summary length 33 is not in 1..32"):
        m.init_matrix(inits, 1)
    m, inits = _one(mamba, lambda p: ir.Exponential(p), n=32)
    m.init_matrix(inits, 1)
    for st in ("var", "std"):
        m, inits = _one(mamba, lambda p: ir.Exponential(p), summary=("mean", st), n=1)
        with pytest.raises(E, match="var and std summaries need data nodes of >= 2 elements"):
            m.init_matrix(inits, 1)
    # scale length, discrete params
    m, inits = _one(mamba, lambda p: ir.Exponential(p))
    m.setsamplers([mamba.ABC("p", [1.0, 2.0], "sum", 0.5)])
    with pytest.raises(E, match="length\\(scale\\) differs from variate length 1"):
        m.init_matrix(inits, 1)
    m = ir.Model(y=ir.Stochastic(1, lambda z: ir.Normal(z, 1.0), False), z=ir.Stochastic(1, lambda: ir.Bernoulli(0.5)))
    m.setsamplers([mamba.ABC("z", 1.0, "sum", 0.5)])
    with pytest.raises(E, match="discrete node z cannot be sampled by ABC"):
        m.init_matrix([{"y": [0.0, 1.0], "z": [0.0, 1.0]}], 1)
    # an observed Uniform whose bounds read a sampled node is simulated by ABC blocks only
    m, inits = _one(mamba, lambda p: ir.Uniform(0.0, p), y=[0.1, 0.2, 0.3])
    m.init_matrix(inits, 1)
    m.setsamplers([mamba.Slice("p", 1.0)])
    with pytest.raises(E, match="Uniform bounds of y must be constants or data"):
        m.init_matrix(inits, 1)


def test_engine_validation(mamba):
    """mmb_ir_jit_prebuild validates the IR and the block specs like mmb_create_ir and needs no device: the test
    models pass and the specialised kernel declines them naming ABC; mmb_create_ir refuses every bad spec."""
    lib, a = mamba.abi.lib(), mamba.abi
    buf = C.create_string_buffer(512)
    for make in (ar.line_abc, ar.caps, ar.wide, ar.families, ar.hierarchical, ar.beta_binomial, ar.beta_bernoulli):
        m = make(mamba, 2)[0]
        spec, I = m.spec(), m.ir()
        rc = lib.mmb_ir_jit_prebuild(C.byref(spec), C.byref(I), buf, 512)
        assert rc == -2 and b"ABC" in buf.value, (make.__name__, rc, buf.value, lib.mmb_last_error(None))

    def rc_of(spec, I):
        h = C.c_void_p()
        rc = lib.mmb_create_ir(C.byref(spec), C.byref(I), 0, C.byref(h))
        assert not h.value
        return rc, lib.mmb_last_error(None).decode()
    bad = [("beta", -0.5, "decay is not in [0, 1]"), ("beta", 1.5, "decay is not in [0, 1]"),
           ("beta", math.nan, "decay is not in [0, 1]"), ("epsilon", 0.0, "epsilon is not finite and > 0"),
           ("epsilon", math.inf, "epsilon is not finite and > 0"), ("batchsize", 0, "maxdraw is not in 1..1024"),
           ("batchsize", 1025, "maxdraw is not in 1..1024"), ("nsteps", 0, "nsim is not in 1..8"),
           ("nsteps", 9, "nsim is not in 1..8"), ("form", 7, "ABC form"), ("form", 7 << 8, "ABC form"),
           ("form", 1 << 17, "ABC form"), ("form", -1, "ABC form"), ("transform", 0, "transform = 1"),
           ("ntuning", 2, "summary codes"), ("ntuning", 11, "summary codes")]
    for field, val, want in bad:
        m = ar.line_abc(mamba, 2)[0]
        spec, I = m.spec(), m.ir()
        setattr(spec.blocks[0], field, val)
        rc, msg = rc_of(spec, I)
        assert rc == -1 and want in msg, (field, val, msg)

    def tuned(make, tuning, block=0):
        m = make(mamba, 2)[0]
        spec, I = m.spec(), m.ir()
        t = np.asarray(tuning, dtype=np.float64)
        spec.blocks[block].ntuning, spec.blocks[block].tuning = t.size, a.dptr(t)
        return rc_of(spec, I)
    for tuning, want in [([0.5, -0.25, 0.0], "ABC scale must be finite and >= 0"),
                         ([0.5, math.nan, 0.0], "ABC scale must be finite and >= 0"),
                         ([0.5, 0.25, 7.0], "unknown summary code"), ([0.5, 0.25, 1.5], "unknown summary code"),
                         ([0.5, 0.25, 0.0, 2.0], "identity summary may only stand alone"),
                         ([0.5, 0.25] + [1.0] * 7, "total summary length is not in 1..32")]:
        rc, msg = tuned(ar.line_abc if len(tuning) < 9 else ar.families, tuning)
        assert rc == -1 and want in msg, (tuning, msg)
    rc, msg = tuned(ar.beta_binomial, [1.0, 2.0, 4.0])  # std of a one-element node
    assert rc == -1 and "var and std summaries need data nodes of >= 2 elements" in msg, msg
    # a Gamma data node and a block with no data node, patched in behind the host's back
    ir = mamba.ir
    m = ir.Model(y=ir.Stochastic(1, lambda p: ir.Gamma(2.0, p), False), p=ir.Stochastic(lambda: ir.Gamma(2.0, 1.0)))
    m.setsamplers([mamba.RWM("p", 1.0)]).init_matrix([{"y": [0.5, 0.5], "p": 0.5}], 1)
    good = ar.beta_binomial(mamba, 1)[0].spec()
    spec, I = m.spec(), m.ir()
    t = np.array([1.0, 1.0])
    for f in ("sampler", "form", "batchsize", "nsteps", "beta", "epsilon", "transform"):
        setattr(spec.blocks[0], f, getattr(good.blocks[0], f))
    spec.blocks[0].ntuning, spec.blocks[0].tuning = 2, a.dptr(t)
    rc, msg = rc_of(spec, I)
    assert rc == -1 and "Gamma data nodes are not supported" in msg, msg
    I.blocks[0].nterms = 1
    rc, msg = rc_of(spec, I)
    assert rc == -1 and "at least one data node" in msg, msg


# ------------------------------------------------------------------ 4. csrc/abc.h against the closed forms
HOST_SRC = r"""
#include "abc.h"
double h_kernel(int kind, double eps, double d) { return mmb_abc_kernel_pdf(kind, eps, d); }
double h_exp_pdf(double eps, double x) { return mmb_abc_exp_pdf(eps, x); }
unsigned h_block(int b, int k, int i, int j) { return mmb_abc_block(b, k, i, j); }
"""


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("abc_host")
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no C compiler: the oracle itself could not have been built"
    src, so = os.path.join(str(tmp), "abc_host.c"), os.path.join(str(tmp), "libabchost.so")
    with open(src, "w") as f:
        f.write(HOST_SRC)
    subprocess.run([cc, "-O2", "-std=gnu99", "-ffp-contract=off", "-fPIC", "-shared", "-I",
                    os.path.join(ROOT, "mamba.jl_amd", "csrc"), "-I", os.path.join(ROOT, "include"), src, "-o", so,
                    "-lm"], check=True)
    L = C.CDLL(so)
    L.h_kernel.restype, L.h_kernel.argtypes = C.c_double, [C.c_int, C.c_double, C.c_double]
    L.h_exp_pdf.restype, L.h_exp_pdf.argtypes = C.c_double, [C.c_double, C.c_double]
    L.h_block.restype, L.h_block.argtypes = C.c_uint, [C.c_int] * 4
    return L


@pytest.mark.parametrize("kind", range(7))
def test_header_kernel_pdfs(host, oracle, kind):
    """The header against the closed forms (a few ulps: libm's exp and cos) and against the restatement (the same
    bits), then its integral over [0, eps] (Normal: [0, 8 eps]) = 1/2 by Simpson's rule."""
    for eps in (1.0, 0.5, 0.1, 3.7):
        for d in list(np.linspace(0.0, 1.25 * eps, 41)) + [eps, np.nextafter(eps, 2 * eps), np.nextafter(eps, 0.0)]:
            got = host.h_kernel(kind, eps, float(d))
            assert got == ar.kernel_pdf(oracle.L, kind, eps, float(d))
            want = ar.kernel_closed_form(kind, eps, float(d))
            assert abs(got - want) <= 8e-16 * max(abs(want), 1.0 / eps), (kind, eps, d, got, want)
        top = 8.0 * eps if kind == 0 else eps
        n = 2000
        xs = np.linspace(0.0, top, n + 1)
        f = np.array([host.h_kernel(kind, eps, float(x)) for x in xs])
        integral = (top / n / 3.0) * (f[0] + f[-1] + 4.0 * f[1:-1:2].sum() + 2.0 * f[2:-1:2].sum())
        # SymUniform's step at the end point is inside the interval: exact; the others are smooth on it
        assert abs(integral - 0.5) < 1e-9, (kind, eps, integral)
    # SymUniform is inclusive at u = 1; every kernel but Normal is 0 beyond it, NaN distances give 0 or NaN
    assert host.h_kernel(1, 0.5, 0.5) == 1.0 and host.h_kernel(1, 0.5, np.nextafter(0.5, 1.0)) == 0.0
    if kind:
        assert host.h_kernel(kind, 1.0, 1.0000001) == 0.0 and host.h_kernel(kind, 1.0, math.nan) == 0.0
    else:
        assert math.isnan(host.h_kernel(0, 1.0, math.nan)) and host.h_kernel(0, 1.0, math.inf) == 0.0


def test_header_exp_pdf_and_blocks(host, oracle):
    for eps, x in ((1.0, 0.0), (0.5, 0.3), (2.0, 9.0)):
        assert host.h_exp_pdf(eps, x) == ar.exp_pdf(oracle.L, eps, x)
        assert abs(host.h_exp_pdf(eps, x) - math.exp(-x / eps) / eps) < 1e-15
    seen = set()
    for b in (0, 3, 7):
        for k in (0, 1, 1024):
            for i in (0, 7):
                for j in (0, 15, 16):
                    assert host.h_block(b, k, i, j) == ar.abc_block(b, k, i, j)
                    seen.add(ar.abc_block(b, k, i, j))
    assert len(seen) == 54


# ------------------------------------------------------------------ 5. the restatement
def test_summaries():
    x = [3.0, -1.5, 0.25, 8.0, 2.0]
    got = ar.summarise(x, [ar.SUM, ar.MEAN, ar.VAR, ar.STD, ar.MINIMUM, ar.MAXIMUM])
    want = [sum(x), np.mean(x), np.var(x, ddof=1), np.std(x, ddof=1), -1.5, 8.0]
    np.testing.assert_allclose(got, want, rtol=1e-15)
    assert ar.summarise(x, [ar.IDENTITY]) == x
    rng = np.random.default_rng(1)
    x = list(rng.normal(size=70))
    got = ar.summarise(x, [ar.SUM, ar.VAR, ar.MINIMUM, ar.MAXIMUM])
    np.testing.assert_allclose(got, [math.fsum(x), np.var(x, ddof=1), min(x), max(x)], rtol=1e-13)
    assert ar.dist([1.0, 2.0, 2.0], [0.0, 0.0, 0.0]) == 3.0


def test_restatement_fixtures_meet_no_threshold(mamba, oracle):
    """The replay fixtures' seeds: no accept uniform within 1e-9 relative of its ratio, so the device is compared
    with no skip at all (tests/test_gpu_abc.py); the first update fills the row and later ones keep its layout."""
    made = ar.line_abc(mamba, 2)
    d, vals, tune, counts, near, skipped = ar.restate(oracle, mamba, made, 11, 3)
    assert near == 0 and d.shape == (3, 3, 2) and tune.shape == (2, 22 + 13)
    assert np.all(tune[:, 0] == 1.0) and np.all(tune[:, 22] == 1.0) and np.all(np.isfinite(tune))
    assert counts[0]["updates"] == counts[1]["updates"] == 6
    # decay = 1: the tolerances never rise above their first values and never fall below epsilon
    assert np.all(tune[:, 16:19] >= 0.5) and np.all(tune[:, 32:35] >= 0.1)
    # a scale of 800 on log(s2): candidates overflow to logprior1 == -Inf and are skipped
    sch = [mamba.ABC("beta", [0.5, 0.25], "identity", 0.5, kernel="Normal", maxdraw=4, nsim=2),
           mamba.ABC("s2", 800.0, ("mean", "std"), 0.1, kernel="Epanechnikov", maxdraw=4, nsim=2)]
    *_, near, skipped = ar.restate(oracle, mamba, ar.line_abc(mamba, 2, sch), 11, 3)
    assert near == 0 and skipped > 0


def test_restatement_exact_posterior(mamba, oracle):
    """p ~ Beta(2, 3), y ~ Binomial(10, p), y = 3, identity, SymUniform, epsilon = 0.5: a simulation within 0.5 of
    y is y itself, so the chain targets the exact posterior Beta(5, 10).  96 chains, 120 iterations, burn-in 40:
    the mean over chains of the per-chain means within 5 SE (the chains' own spread) of 1/3."""
    K, iters, burn = 96, 120, 40
    made = ar.beta_binomial(mamba, K, nsim=1)
    d, vals, tune, counts, near, _ = ar.restate(oracle, mamba, made, 5, iters, burnin=burn)
    means = d[:, 0, :].mean(axis=0)
    se = means.std(ddof=1) / math.sqrt(K)
    z = (means.mean() - 1.0 / 3.0) / se
    print(f"restatement exact posterior: mean {means.mean():.4f} se {se:.4f} z {z:+.2f} "
          f"accept {counts[0]['accepts'] / counts[0]['updates']:.3f}")
    assert abs(z) < 5.0
    assert 0.02 < counts[0]["accepts"] / counts[0]["updates"] < 0.9
