"""ABC (src/samplers/abc.jl:23-147) on the GPU against the Python restatement of the update (tests/abc_ref.py) on
identical Philox streams: draws, final values, full tune rows and the update / accept counts identical, zero
differing bits, with no accept decision near its threshold (asserted, so nothing is skipped) -- then windows, chain
shards, tune rows set and continued, checkpoints, two models whose ABC target is the exact posterior, and the
refusals."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import abc_ref as ar

pytestmark = pytest.mark.gpu
SEED, K, ITERS = 11, 7, 5   # seven chains: three full waves of two chains and a half-filled one


def _mb():
    import _mamba_path
    return _mamba_path.load()


def _oracle():
    import oracle_lib
    return oracle_lib.Oracle()


def _line(**kw):
    def make(mb, k):
        kw2 = {"maxdraw": 3, "nsim": 2, **kw}
        return ar.line_abc(mb, k, [mb.ABC("beta", [0.5, 0.25], "identity", 0.5, kernel="Normal", **kw2),
                                   mb.ABC("s2", 0.5, ("mean", "std"), 0.1, kernel="Epanechnikov", **kw2)])
    return make


def _kernel(i):
    return lambda mb, k: ar.line_abc(mb, k, ar.kernel_scheme(mb, i))


def _defaults(mb, k):
    return ar.line_abc(mb, k, [mb.ABC("beta", [0.5, 0.25], "identity", 0.5), mb.ABC("s2", 0.5, ("mean", "std"), 0.1)])


def _overflow(mb, k):
    """A scale of 800 on log(s2): some candidates overflow to logprior1 == -Inf and are skipped."""
    return ar.line_abc(mb, k, [mb.ABC("beta", [0.5, 0.25], "identity", 0.5, kernel="Normal", maxdraw=4, nsim=2),
                               mb.ABC("s2", 800.0, ("mean", "std"), 0.1, kernel="Epanechnikov", maxdraw=4, nsim=2)])


CASES = {"line_abc": ar.line_abc, "defaults": _defaults, "decay0": _line(decay=0.0), "decay075": _line(decay=0.75),
         "decay1": _line(decay=1.0), "randeps": _line(randeps=True, decay=0.75), "caps": ar.caps, "wide": ar.wide,
         "families": ar.families, "overflow": _overflow,
         **{f"kernel-{ar.KERNELS[i]}": _kernel(i) for i in range(7)}}


@functools.lru_cache(maxsize=None)
def reference(case, k=K, iters=ITERS):
    """The whole run restated once: (draws, values, tune rows, counts, near, skipped)."""
    return ar.restate(_oracle(), _mb(), CASES[case](_mb(), k), SEED, iters)


def engine_run(case, k=K, windows=(ITERS,), chain_offset=0, rows=None):
    mb = _mb()
    m, V, *_ = CASES[case](mb, k if rows is None else max(k, rows.stop))
    eng = mb.Engine(m)
    eng.init_chains(V if rows is None else V[rows], chain_offset=chain_offset, seed=SEED)
    d = np.concatenate([eng.run(w) for w in windows], axis=0)
    out = d, eng.values().copy(), eng.tune().copy(), eng.accept_stats()
    eng.close()
    return out


def counts_of(stats):
    return {b: (v["updates"], v["accepts"]) for b, v in stats.items()}


# ---- 1. replays, bit for bit: values and full tune rows
@pytest.mark.parametrize("case", list(CASES))
def test_replay(case):
    d, vals, tune, counts, near, skipped = reference(case)
    assert near == 0, "the fixture's seed puts an accept uniform within 1e-9 of its ratio: choose another"
    if case == "overflow":
        assert skipped > 0
    dg, vg, tg, sg = engine_run(case)
    np.testing.assert_array_equal(dg, d)
    np.testing.assert_array_equal(vg, vals)
    np.testing.assert_array_equal(tg, tune)
    assert counts_of(sg) == counts_of(counts)
    assert all(v["updates"] == K * ITERS for v in sg.values())


def test_replay_hierarchical():
    """The data node theta is sampled by the AMWG block that follows: every ABC update is replayed from the device's
    own pre-update row (theta's values are the device's), so Tobs moves between iterations; the ABC block's values
    and its tune rows bit for bit."""
    mb = _mb()
    made = ar.hierarchical(mb, K)
    m, V = made[0], made[1]
    assert m.monitor_names == ["mu"] + [f"theta[{i + 1}]" for i in range(4)]
    eng = mb.Engine(m)
    eng.init_chains(V, seed=SEED)
    dg = eng.run(6)
    tg, sg = eng.tune(), eng.accept_stats()
    eng.close()
    R = ar.restatement(_oracle(), mb, made, SEED)
    tune = np.zeros((K, R.tune_len(0)))
    assert R.replay(0, V, dg, tune) == 0 and R.near == 0
    np.testing.assert_array_equal(tg[:, :R.tune_len(0)], tune)
    assert counts_of(sg) == counts_of(R.stats_counts())
    assert len({float(x) for x in dg[:, 1, 0]}) > 1   # theta moved


# ---- 2. windows and chain shards
def test_windows_and_chain_shards():
    whole = engine_run("line_abc", k=8, windows=(6,))
    split = engine_run("line_abc", k=8, windows=(2, 4))
    for a, b in zip(whole[:3], split[:3]):
        np.testing.assert_array_equal(a, b)
    assert counts_of(whole[3]) == counts_of(split[3])
    lo = engine_run("line_abc", k=8, windows=(6,), rows=slice(0, 3))
    hi = engine_run("line_abc", k=8, windows=(6,), rows=slice(3, 8), chain_offset=3)
    np.testing.assert_array_equal(np.concatenate([lo[0], hi[0]], axis=2), whole[0])
    np.testing.assert_array_equal(np.concatenate([lo[1], hi[1]], axis=0), whole[1])
    np.testing.assert_array_equal(np.concatenate([lo[2], hi[2]], axis=0), whole[2])
    assert {b: (lo[3][b]["updates"] + hi[3][b]["updates"], lo[3][b]["accepts"] + hi[3][b]["accepts"]) for b in lo[3]} == \
        counts_of(whole[3])


# ---- 3. tune rows read, set and continued; checkpoints
def test_tune_rows_set_and_continue(tmp_path):
    mb = _mb()
    d, vals, tune, counts, near, _ = reference("randeps", K, 6)
    assert near == 0
    m, V, *_ = CASES["randeps"](mb, K)
    eng = mb.Engine(m)
    eng.init_chains(V, seed=SEED)
    assert not eng.tune().any()   # zeroed: `initialised` is 0 in every chain
    d1 = eng.run(2)
    t2, v2 = eng.tune().copy(), eng.values().copy()
    eng.set_tune(t2)
    np.testing.assert_array_equal(eng.tune(), t2)
    bad = t2.copy()
    bad[1, 0] = 0.5
    with pytest.raises(Exception, match="initialised 0 or 1"):
        eng.set_tune(bad)
    eng.close()
    m2, _, *_ = CASES["randeps"](mb, K)
    e2 = mb.Engine(m2)
    e2.init_chains(v2, seed=SEED)
    e2.set_tune(t2)
    e2.set_iter(2)
    d2 = e2.run(4, burnin=2)
    np.testing.assert_array_equal(np.concatenate([d1, d2], axis=0), d)
    np.testing.assert_array_equal(e2.values(), vals)
    np.testing.assert_array_equal(e2.tune(), tune)
    e2.close()
    # write / read / mcmc_restart against the unbroken run
    m3, V3, *_ = CASES["randeps"](mb, K)
    part = mb.mcmc(m3, mb.ir.line_abc_inputs(), mb.ir.line_abc_inits(K, 1), 2, chains=K, seed=SEED)
    np.testing.assert_array_equal(m3.init_matrix(mb.ir.line_abc_inits(K, 1), K), V3)
    name = os.path.join(str(tmp_path), "abc.ckpt")
    mb.write(name, part)
    part.engine.close()
    m4, *_ = CASES["randeps"](mb, K)
    back = mb.mcmc_restart(mb.read(name, model=m4), 4)
    np.testing.assert_array_equal(back.value, d)
    np.testing.assert_array_equal(back.engine.values(), vals)
    np.testing.assert_array_equal(back.engine.tune(), tune)
    back.engine.close()


# ---- 4. the exact posterior
def _posterior(make, exact_mean):
    mb = _mb()
    Kp, iters, burn = 2048, 300, 100
    m, V, *_ = make(mb, Kp)
    eng = mb.Engine(m)
    eng.init_chains(V, seed=SEED)
    d = eng.run(iters, burnin=burn)
    st = eng.accept_stats()
    eng.close()
    means = d[:, 0, :].mean(axis=0)
    se = means.std(ddof=1) / math.sqrt(Kp)
    z = (means.mean() - exact_mean) / se
    print(f"{make.__name__}: mean {means.mean():.5f} exact {exact_mean:.5f} se {se:.5f} z {z:+.2f} "
          f"accept rate {st[0]['rate']:.3f}")
    assert abs(z) < 5.0


def test_exact_posterior_beta_binomial():
    """p ~ Beta(2, 3), y ~ Binomial(10, p), y = 3, identity, nsim = 2, SymUniform, epsilon = 0.5, decay = 1,
    maxdraw = 1: the posterior is Beta(5, 10); 2048 chains, 300 iterations, burn-in 100."""
    _posterior(ar.beta_binomial, 5.0 / 15.0)


def test_exact_posterior_beta_bernoulli():
    """y[8] ~ Bernoulli(p) with three ones, "sum", nsim = 1: the posterior is Beta(5, 8)."""
    _posterior(ar.beta_bernoulli, 5.0 / 13.0)


# ---- 5. kernel selection and the refusals through the C ABI
def test_decline_by_name_and_engine_refusals():
    mb = _mb()
    m, V, *_ = ar.line_abc(mb, 4)
    eng = mb.Engine(m)
    eng.init_chains(V, seed=SEED)
    eng.run(2)
    jit, info = eng.ir_jit()
    eng.close()
    assert not jit and "ABC" in info, info
    lib = mb.abi.lib()
    for field, val, want in [("beta", 1.5, "decay is not in [0, 1]"), ("epsilon", -1.0, "epsilon is not finite"),
                             ("batchsize", 2000, "maxdraw is not in 1..1024"), ("nsteps", 9, "nsim is not in 1..8"),
                             ("form", 9, "ABC form"), ("ntuning", 1, "summary codes")]:  # (block 1: scale[1], no code left)
        m, *_ = ar.line_abc(mb, 2)
        spec, I = m.spec(), m.ir()
        setattr(spec.blocks[1], field, val)
        h = C.c_void_p()
        rc = lib.mmb_create_ir(C.byref(spec), C.byref(I), 0, C.byref(h))
        assert rc == -1 and not h.value and want in lib.mmb_last_error(None).decode(), (field, val)
