"""SliceSimplex blocks and Dirichlet nodes on the device against the restatement (tests/slicesimplex_ref.py).

The replay's candidates and accepted draws are bit-equal to the device's; the one decision that may differ
is logf(x) < p0 within slicesimplex_ref.DELTA_REL of the threshold (at most 2 such updates per test;
tests/test_slicesimplex.py shows the restatement alone meets none on these seeds).  All runs: thin 1,
burnin 0, every sampled node monitored.
"""
import functools
import json
import math
import os

import numpy as np
import pytest

import slicesimplex_ref as ref

pytestmark = pytest.mark.gpu
SEED = 11
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _mb():
    import _mamba_path
    return _mamba_path.load()


def _prim():
    import oracle_lib
    return ref.Prim(oracle_lib.Oracle().L)


def scheme(name, mb):
    if name == "A":
        return [mb.SliceSimplex("P")]
    if name == "B":
        return [mb.SliceSimplex("P", scale=ref.MB_SCALE)]
    s = mb.ir.eyes_scheme()
    assert s[3].scale == ref.MC_SCALE
    return s[::-1] if name == "Cr" else s


def build(name, K):
    mb = _mb()
    m, inputs, inits = getattr(ref, "model" + name[0])(mb.ir)
    m.setinputs(inputs).setsamplers(scheme(name, mb))
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


def init_rows(name, V, d):
    """The chains' initial values in monitored-column order (a Logical's columns are not state: left 0)."""
    m, _ = build(name, V.shape[0])
    rows = np.zeros((V.shape[0], d.shape[1]))
    col = 0
    for n in m.order:
        if not m.defs[n].monitor:
            continue
        ln = m.ir().nodes[m.order.index(n)].len
        if n in m.params:
            rows[:, col:col + ln] = V[:, m.nodes[n].offset:m.nodes[n].offset + ln]
        col += ln
    return rows


def replay(name, spec, K, iters):
    d, V, _ = cached(name, K, iters)
    R = ref.Replay(_prim(), spec, SEED).run(init_rows(name, V, d), d)
    print(f"{name}: {R.updates} updates, {R.cands / R.updates:.2f} candidates per update, {R.skips} threshold skips, "
          f"{len(R.mismatch)} mismatches")
    assert R.mismatch == []
    assert R.skips <= 2
    assert R.updates == K * iters
    return R


# ---- model A: three categories, T observed
def test_modelA_replay():
    replay("A", ref.specA(), 8, 200)
    d, _, _ = cached("A", 8, 200)
    assert len(np.unique(d[:, 0, :])) > 1000  # the chains move
    assert np.abs(d.sum(axis=1) - 1.0).max() < 1e-12 and d.min() >= 0.0


def test_modelA_exact_posterior():
    """4096 independent chains, 30 updates, the last draw only, against Dirichlet(alpha + counts) =
    Dirichlet([8, 5, 2.5]): each coordinate's mean within 5 standard errors sqrt(var / 4096), and its mean
    squared deviation from the exact mean within 5 sqrt(2) var / sqrt(4096) of the exact variance."""
    K = 4096
    mb = _mb()
    m, V = build("A", K)
    eng = mb.Engine(m)
    eng.init_chains(V, seed=SEED)
    d = eng.run(30, burnin=29)
    eng.close()
    assert d.shape == (1, 3, K)
    a0 = math.fsum(ref.MA_POST)
    for i, a in enumerate(ref.MA_POST):
        mean = a / a0
        var = a * (a0 - a) / (a0 * a0 * (a0 + 1.0))
        x = d[0, i, :]
        zm = (x.mean() - mean) / math.sqrt(var / K)
        msd = float(((x - mean) ** 2).mean())
        zv = (msd - var) / (math.sqrt(2.0) * var / math.sqrt(K))
        print(f"P[{i + 1}]: mean {x.mean():.5f} (exact {mean:.5f}, {zm:+.2f} se), "
              f"mean squared deviation {msd:.6f} (exact {var:.6f}, {zv:+.2f} units)")
        assert abs(x.mean() - mean) <= 5.0 * math.sqrt(var / K)
        assert abs(msd - var) <= 5.0 * math.sqrt(2.0) * var / math.sqrt(K)


# ---- model B: a full lane group, T longer than one
def test_modelB_replay():
    R = replay("B", ref.specB(), 4, 100)
    assert R.cands > 4 * R.updates  # the shrink runs, many times per update at k = 32


# ---- model C: eyes with 6 observations, the reference's scheme in both orders
@pytest.mark.parametrize("name,reverse", [("C", False), ("Cr", True)])
def test_modelC_replay(name, reverse):
    d, _, _ = cached(name, 4, 200)
    n = len(ref.MC_Y)
    assert len(np.unique(d[:, :n, :])) == 2  # T visits both components: P's conditional changes
    replay(name, ref.specC(reverse), 4, 200)


# ---- stream hygiene
def test_windows_and_chain_offset():
    d, V, _ = cached("C", 8, 200)
    d2, _, _ = run("C", 8, 200, windows=[70, 130])
    np.testing.assert_array_equal(d2, d)
    db, _, _ = run("C", 3, 200, chain_offset=5, init=V[5:])
    np.testing.assert_array_equal(db, d[:, :, 5:])


# ---- model statistics
def test_logpdf_and_predict():
    mb = _mb()
    m, inputs, inits = ref.modelA(mb.ir)
    m.setsamplers([mb.SliceSimplex("P")])
    K, n = 4, 50
    sim = mb.mcmc(m, inputs, inits(K), n, chains=K, seed=SEED, keep_device=True)
    assert sim.value.shape == (n, 3, K)
    lp = sim.logpdf(["P", "T"]).value
    worst = 0.0
    for i in range(n):
        for k in range(K):
            want, mag = ref.modelA_logpdf(sim.value[i, :, k])
            worst = max(worst, abs(lp[i, 0, k] - want) / mag)
            assert abs(lp[i, 0, k] - want) <= 1e-12 * mag
    print(f"logpdf: worst error {worst:.2e} of the sum of absolute terms")
    with pytest.raises(mb.ArgumentError, match="Categorical that reads"):
        sim.predict(["T"])


# ---- the specialised kernel declines
def test_ir_jit_declines():
    for name in ("A", "C"):
        _, _, (jit, info) = cached(name, 8, 200)
        assert not jit and "interpreter" in info and "SliceSimplex" in info, info


# ---- eyes as published
def test_eyes_published():
    """doc/examples/eyes.jl as published (eyes.rst:39-50): 64 chains from the reference's two inits, 10000
    iterations, burnin 2500, thin 2; |ours - published| < 5 published MCSE + 4 of our own SE, the rule of
    test_gpu_ir.test_ir_published_summaries."""
    g = json.load(open(os.path.join(GOLD, "eyes_published.json")))
    first, last = (int(t) for t in g["iterations"].split(":"))
    mb = _mb()
    ir = mb.ir
    K = 64
    m = ir.eyes_model()
    m.setinputs(ir.eyes_inputs()).setsamplers(ir.eyes_scheme())
    two = ir.eyes_inits()
    V = m.init_matrix([two[c % 2] for c in range(K)], K)
    eng = mb.Engine(m)
    eng.init_chains(V, seed=2026)
    d = eng.run(last, burnin=first - 2, thin=g["thin"])
    eng.close()
    assert d.shape[0] == (last - first) // 2 + 1
    seen = 0
    for j, nm in enumerate(m.monitor_names):
        pub = g["rows"].get(nm.replace("lam[", "lambda["))
        if pub is None:
            continue
        seen += 1
        cm = d[:, j, :].mean(axis=0)
        est, se = float(cm.mean()), float(cm.std(ddof=1) / np.sqrt(cm.size))
        tol = 5.0 * pub["mcse"] + 4.0 * se
        print(f"{nm}: ours {est:.5f} (se {se:.5f}), published {pub['mean']:.5f} (mcse {pub['mcse']:.5f}), "
              f"|diff| {abs(est - pub['mean']):.5f}, tol {tol:.5f}")
        assert abs(est - pub["mean"]) < tol, (nm, est, pub["mean"], tol)
    assert seen == 5
