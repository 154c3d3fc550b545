"""RWM (src/samplers/rwm.jl:49-71) on the CPU: the constructor and its spec, the proposal samplers
of the restatement (tests/rwm_ref.py) against their closed-form cdfs and against csrc/symdist.h
compiled for the host, and the restatement itself against the exact posterior of the line model."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import rwm_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")
KINDS = {"SymUniform": 1, "SymTriangularDist": 2, "Epanechnikov": 3, "Biweight": 4, "Triweight": 5, "Cosine": 6}


def test_constructor(mamba):
    abi = mamba.abi
    assert abi.MMB_SAMPLER_RWM == 8 and abi.MMB_ABI_VERSION == 10
    s = mamba.RWM("beta", 0.5)
    assert (s.kind, s.form, s.transform, s.adapt) == (8, abi.MMB_RWM_NORMAL, 1, abi.MMB_ADAPT_NONE)
    assert repr(s) == "RWM(['beta'])"
    for i, name in enumerate(["Normal", "SymUniform", "SymTriangularDist", "Epanechnikov", "Biweight", "Triweight",
                              "Cosine"]):
        assert getattr(mamba, name) == name
        assert mamba.RWM("beta", 1.0, getattr(mamba, name)).form == i
        assert mamba.RWM("beta", 1.0, ":" + name.lower()).form == i
    with pytest.raises(mamba.ArgumentError, match="unsupported proposal"):
        mamba.RWM("beta", 1.0, "Laplace")
    with pytest.raises(mamba.ArgumentError, match="scale"):
        mamba.RWM("beta", -1.0)
    with pytest.raises(mamba.ArgumentError, match="scale"):
        mamba.RWM("beta", [1.0, np.inf])
    m = mamba.line()
    with pytest.raises(mamba.ArgumentError, match=r"length\(scale\) differs from variate length 2"):
        m.setsamplers([mamba.RWM("beta", [1.0, 2.0, 3.0])])
    with pytest.raises(mamba.ArgumentError, match=r"length\(scale\) differs from variate length 3"):
        m.setsamplers([mamba.RWM(["beta", "s2"], [1.0, 2.0])])


def test_spec_packing(mamba):
    m = mamba.line().setsamplers([mamba.RWM("beta", [1.0, 0.4]), mamba.RWM("s2", 1.5, mamba.Epanechnikov)])
    sp = m.spec()
    b0, b1 = sp.blocks[0], sp.blocks[1]
    assert (b0.sampler, b0.form, b0.transform, b0.adapt, b0.dim, b0.ntuning) == (8, 0, 1, mamba.abi.MMB_ADAPT_NONE, 2, 2)
    assert [b0.tuning[i] for i in range(2)] == [1.0, 0.4]
    assert (b1.sampler, b1.form, b1.transform, b1.dim, b1.ntuning) == (8, 3, 1, 1, 1)
    # a scalar scale is broadcast to the variate length by the host
    r = mamba.rats().setsamplers([mamba.RWM("alpha", 0.25, mamba.Cosine), mamba.RWM(["mu_beta", "s2_beta"], 0.5)])
    sp = r.spec()
    assert (sp.blocks[0].dim, sp.blocks[0].ntuning, sp.blocks[0].form) == (30, 30, 6)
    assert [sp.blocks[0].tuning[i] for i in range(30)] == [0.25] * 30
    assert (sp.blocks[1].dim, sp.blocks[1].ntuning) == (2, 2)
    assert [sp.blocks[1].tuning[i] for i in range(2)] == [0.5, 0.5]


def test_tune_len_arithmetic(mamba, oracle):
    """An RWM block's tune row is scale[d]: the restatement's rows are the scheme's scales, block by
    block, next to the other kinds' lengths (AMWG 2 + 2d as the oracle counts it)."""
    m = mamba.rats().setinputs(mamba.model.RATS_DATA)
    scheme = [mamba.RWM("s2_c", 0.3, mamba.Cosine), mamba.RWM("alpha", 1.0),
              mamba.RWM(["mu_alpha", "s2_alpha"], [3.0, 0.5], mamba.Triweight)]
    m.setsamplers(scheme)
    tw = mamba.rats().setinputs(mamba.model.RATS_DATA).setsamplers(rwm_ref.twin_scheme(mamba, scheme))
    R = rwm_ref.Restatement(oracle, mamba, m, tw, seed=1)
    sc = R.scales0(3)
    t = R.tune(sc, 3)
    assert t.shape == (3, 1 + 30 + 2)
    np.testing.assert_array_equal(t[1], [0.3] + [1.0] * 30 + [3.0, 0.5])
    st = oracle.new_state(tw, mamba.model.rats_init_ls(3))
    assert st["tl"] == (2 + 2 * 1) + (2 + 2 * 30) + (2 + 2 * 2)


def test_create_validates_the_kind(mamba):
    """mmb_create refuses a malformed RWM block before it touches a device: ntuning != dim, a scale
    that is negative or not finite, a proposal out of range (MMB_E_ARG), and RWM on logistic
    (MMB_E_UNSUPPORTED)."""
    abi = mamba.abi
    lib = abi.lib()

    def create(model, mutate):
        sp = model.spec()
        keep = mutate(sp.blocks[0])
        h = C.c_void_p()
        rc = lib.mmb_create(C.byref(sp), 0, C.byref(h))
        assert not h.value
        del keep
        return rc, (lib.mmb_last_error(None) or b"").decode()

    def line():
        return mamba.line().setsamplers([mamba.RWM("beta", [1.0, 0.4])])

    def short(b):
        b.ntuning = 1
    rc, msg = create(line(), short)
    assert rc == -1 and "length(scale) differs from variate length 2" in msg

    def scale(v):
        def f(b):
            t = np.array([1.0, v])
            b.tuning = abi.dptr(t)
            return t
        return f
    for v in (-0.5, np.inf, np.nan):
        rc, msg = create(line(), scale(v))
        assert rc == -1 and "scale[1]" in msg, (v, rc, msg)

    def prop(b):
        b.form = 7
    rc, msg = create(line(), prop)
    assert rc == -1 and "proposal" in msg
    lg = mamba.logistic(100, 3).setsamplers([mamba.RWM("beta", 0.1)])
    rc, msg = create(lg, lambda b: None)
    assert rc == -2, (rc, msg)


def _variates(oracle, kind):
    return np.array([rwm_ref.symdist(oracle.L, kind, 7, q // 16, 1, 0, q % 16) for q in range(4096)])


@pytest.mark.parametrize("name", sorted(KINDS))
def test_proposal_cdf(oracle, name):
    """4096 variates (seed 7, iteration 1, block 0, chain q // 16, coordinate q % 16): all in
    [-1, 1], Kolmogorov-Smirnov D sqrt(N) < 2.23 (the 1e-4 level) against the closed-form cdf."""
    z = _variates(oracle, KINDS[name])
    assert z.min() >= -1.0 and z.max() <= 1.0
    zs = np.sort(z)
    n = zs.size
    F = rwm_ref.cdf(KINDS[name], zs)
    D = max(np.max(np.arange(1, n + 1) / n - F), np.max(F - np.arange(0, n) / n))
    print(name, "D sqrt(N) =", D * np.sqrt(n))
    assert D * np.sqrt(n) < 2.23


HOST_SRC = r"""
#include "symdist.h"
double sym_variate(int kind, uint64_t seed, uint32_t chain, uint32_t it, uint32_t block, uint32_t k) {
  mmb_rng s = mmb_rng_make(seed, chain, it, block, MMB_SUB_PROPOSAL);
  return mmb_symdist(kind, &s, k);
}
"""


def test_symdist_header_host_bits(oracle, tmp_path):
    """csrc/symdist.h compiled for the host (plain C, -ffp-contract=off) returns the restatement's
    variates bit for bit: the text the kernels compile is what the checker restates."""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler: the oracle itself could not have been built")
    src = tmp_path / "sym_host.c"
    src.write_text(HOST_SRC)
    so = tmp_path / "libsymhost.so"
    subprocess.run([cc, "-O2", "-std=c99", "-ffp-contract=off", "-fPIC", "-shared", "-I",
                    os.path.join(ROOT, "mamba.jl_amd", "csrc"), str(src), "-o", str(so), "-lm"], check=True)
    L = C.CDLL(str(so))
    L.sym_variate.restype = C.c_double
    L.sym_variate.argtypes = [C.c_int, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
    for kind in sorted(KINDS.values()):
        ref = _variates(oracle, kind)
        got = np.array([L.sym_variate(kind, 7, q // 16, 1, 0, q % 16) for q in range(4096)])
        np.testing.assert_array_equal(got, ref)
    assert np.isnan(L.sym_variate(0, 7, 0, 1, 0, 0))  # Normal is not drawn here


def test_restatement_line_posterior(mamba, oracle):
    """The restatement on the node-IR line model, RWM(beta, [1.0, 0.4]) + RWM(s2, 1.5, Epanechnikov),
    32 chains x 3000 iterations (first 500 dropped), seed 11: posterior means within 4 between-chain
    standard errors of the exact ones (tests/golden/line_posterior.json)."""
    post = json.load(open(os.path.join(GOLD, "line_posterior.json")))
    ir = mamba.ir
    K = 32

    def make(scheme):
        m = ir.line_model().setinputs(mamba.model.LINE_DATA)
        m.setsamplers(scheme)
        v = mamba.model.line_init_matrix(K)
        return m, m.init_matrix([{"y": [1.0, 3, 3, 3, 5], "beta": v[k, :2], "s2": v[k, 2]} for k in range(K)], K)

    scheme = [mamba.RWM("beta", [1.0, 0.4]), mamba.RWM("s2", 1.5, mamba.Epanechnikov)]
    m, V = make(scheme)
    tw, _ = make(rwm_ref.twin_scheme(mamba, scheme))
    R = rwm_ref.Restatement(oracle, mamba, m, tw, seed=11)
    d = R.run(V.copy(), 3000, burnin=500, thin=1)
    assert d.shape == (2500, 3, K) and m.monitor_names == ["beta[1]", "beta[2]", "s2"]
    st = R.stats()
    rates = [st[b]["accepts"] / st[b]["updates"] for b in (0, 1)]
    print("acceptance", rates)
    assert all(0.1 < r < 0.9 for r in rates)
    for j, key in enumerate(["E_beta1", "E_beta2", "E_s2"]):
        cm = d[:, j, :].mean(axis=0)
        est, se = float(cm.mean()), float(cm.std(ddof=1) / np.sqrt(K))
        print(key, est, "+-", se, "exact", post[key])
        assert abs(est - post[key]) < 4.0 * se, (key, est, se, post[key])
