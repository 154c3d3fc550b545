"""BMG, BMC3 and BIA blocks on the device against the plain-Python restatement (tests/binary_ref.py).

Replay checks are decision-exact away from thresholds: every new value equals the restatement's, except where a
uniform lies within binary_ref.DELTA of its threshold (at most 2 such updates per test; tests/test_binary.py shows
the restatement alone meets none on these seeds and chain counts).  All runs: thin 1, burnin 0, every sampled node
monitored; the cases and their chain and iteration counts are binary_ref.REPLAY_CASES.
"""
import functools
import itertools
import math

import numpy as np
import pytest

import binary_ref as br

pytestmark = pytest.mark.gpu
SEED = 11


def _mb():
    import _mamba_path
    return _mamba_path.load()


def _uniform():
    import oracle_lib
    return oracle_lib.Oracle().L.orc_uniform


def sampler(mb, kind, k, **kw):
    if kind == "bia":
        return mb.BIA("gamma", **kw)
    return (mb.BMG if kind == "bmg" else mb.BMC3)("gamma", k=k)


def scheme(mb, kind, k, mixed=False, first=True):
    s = [sampler(mb, kind, k)]
    if not mixed:
        return s
    others = [mb.RWM("beta", 0.3), mb.Slice("s2", 1.0, transform=True)]
    return s + others if first else others + s


def build(dn, kind, k, K, mixed=False, first=True):
    mb = _mb()
    m, inputs, inits = br.model(mb.ir, getattr(br, dn), br.prior_of(dn), mixed)
    m.setinputs(inputs).setsamplers(scheme(mb, kind, k, mixed, first))
    return m, m.init_matrix(inits(K), K)


def run(dn, kind, k, K, iters, mixed=False, first=True, chain_offset=0, windows=None, init=None, tune=False):
    """(draws [iters, pmon, K], init matrix, jit info, accept stats, tune rows after the run) of one engine."""
    mb = _mb()
    m, V = build(dn, kind, k, K, mixed, first)
    if init is not None:
        V = init
    eng = mb.Engine(m)
    eng.init_chains(V, chain_offset=chain_offset, seed=SEED)
    d = np.concatenate([eng.run(w) for w in (windows or [iters])], axis=0)
    out = d, V, eng.ir_jit(), eng.accept_stats(), eng.tune() if tune else None
    eng.close()
    return out


@functools.lru_cache(maxsize=None)
def cached(dn, kind, k, K, iters, mixed=False, first=True):
    return run(dn, kind, _thaw(k), K, iters, mixed, first)


def _freeze(k):
    return k if isinstance(k, int) else tuple(tuple(ix) for ix in k)


def _thaw(k):
    return k if isinstance(k, int) else [list(ix) for ix in k]


def replay(dn, kind, k, K, iters, mixed=False, first=True):
    d, V, _, stats, _ = cached(dn, kind, _freeze(k), K, iters, mixed, first)
    sp = br.spec(getattr(br, dn), kind, k, mixed, first)
    R = br.Replay(_uniform(), sp, SEED).run(V, d)
    print(f"{dn} {kind} k={k}: {R.updates} updates, {R.accepts} accepts, {R.skips} threshold skips, "
          f"{len(R.mismatch)} mismatches")
    assert R.mismatch == []
    assert R.skips <= 2
    assert R.updates == K * iters
    b = 0 if first or not mixed else 2
    assert stats[b]["updates"] == K * iters
    assert abs(stats[b]["accepts"] - R.accepts) <= R.skips
    return R, sp


# ---- 1. replay of BMC3 and BMG: int k, the list form, 32 elements (every lane, bit 31), the n = 1 branch
@pytest.mark.parametrize("dn,kind,k,K,iters", br.REPLAY_CASES, ids=[
    f"{c[0]}-{c[1]}-{'lists' if isinstance(c[2], list) else c[2]}-K{c[3]}" for c in br.REPLAY_CASES])
def test_replay(dn, kind, k, K, iters):
    R, _ = replay(dn, kind, k, K, iters)
    d = cached(dn, kind, _freeze(k), K, iters)[0]
    assert set(np.unique(d)) <= {0.0, 1.0}
    assert len(np.unique(d.reshape(iters, -1), axis=0)) > 1  # the chains move
    if dn == "S1":  # no accept step: every update counts as accepted
        assert R.accepts == K * iters


# ---- 2. BIA: one iteration per window, the tune row read after each
@pytest.mark.parametrize("dn,kind,k,K,iters", br.BIA_CASES, ids=[c[0] for c in br.BIA_CASES])
def test_bia_replay(dn, kind, k, K, iters):
    mb = _mb()
    m, V = build(dn, "bia", 1, K)
    n = getattr(br, dn).n
    eng = mb.Engine(m)
    eng.init_chains(V, seed=SEED)
    tunes, draws = [eng.tune().copy()], []
    assert tunes[0].shape == (K, 1 + 2 * n)
    np.testing.assert_array_equal(tunes[0], np.array([[0.0] + [1.0 / n] * (2 * n)] * K))
    for _ in range(iters):
        draws.append(eng.run(1))
        tunes.append(eng.tune().copy())
    # set_tune of a changed row, then get_tune: exact
    t2 = tunes[-1].copy()
    t2[:, 0] += 3.0
    t2[:, 1:] = 0.25 + 0.5 * t2[:, 1:]
    eng.set_tune(t2)
    np.testing.assert_array_equal(eng.tune(), t2)
    stats = eng.accept_stats()
    eng.close()
    d = np.concatenate(draws, axis=0)
    sp = br.spec(getattr(br, dn), "bia")
    R = br.Replay(_uniform(), sp, SEED).run(V, d, tunes=[[list(r) for r in t] for t in tunes])
    print(f"{dn} bia: {R.updates} updates, {R.accepts} accepts, {R.skips} skips, worst A / D error {R.tune_err:.2e}")
    assert R.mismatch == [] and R.skips <= 2 and R.updates == K * iters
    # A and D: the one step from the device's previous row; its inexact inputs are alpha (which inherits the
    # 1e-10 bound on the log densities) and the one-ulp log and exp: two orders of margin, as for DELTA
    assert R.tune_err <= 1e-8
    assert np.all(tunes[-1][:, 0] == iters)
    assert stats[0]["updates"] == K * iters and abs(stats[0]["accepts"] - R.accepts) <= R.skips
    assert 0 < R.accepts


# ---- 3. the binary block mixed with RWM and Slice, in both block orders
@pytest.mark.parametrize("first", [True, False])
def test_mixed_scheme_replay(first):
    d = cached("MIX", "bmg", 2, 8, 200, True, first)[0]
    assert len(np.unique(d[:, 3:6, :])) > 100 and len(np.unique(d[:, 6, :])) > 100  # beta and s2 move
    replay("MIX", "bmg", 2, 8, 200, True, first)


# ---- 4. p_i rounds to 1 and to 0: the 0.5 replacement
def test_edge_replay():
    R, sp = replay(*br.EDGE_CASE)
    assert R.skips == 0
    halves = sp.blocks[0][1].halves
    print(f"EDGE: the 0.5 branch was taken {halves} times")
    assert halves > 0


# ---- 5. the exact posterior
@pytest.mark.parametrize("kind", ["bmg", "bmc3", "bia"])
def test_exact_posterior(kind):
    """S3, 4096 independent chains, 30 iterations, the last one only: the pooled frequencies of the 8 states against
    the enumerated posterior within 5 standard errors sqrt(p (1 - p) / 4096) (the rule of test_bernoulli_exact_posterior)."""
    K = 4096
    mb = _mb()
    m, V = build("S3", kind, 1, K)
    eng = mb.Engine(m)
    eng.init_chains(V, seed=SEED)
    d = eng.run(30, burnin=29)
    eng.close()
    assert d.shape == (1, 3, K)
    states = list(itertools.product([0.0, 1.0], repeat=3))
    lp = [br.logpdf_gamma_y(br.S3, list(g))[0] for g in states]
    mx = max(lp)
    w = [math.exp(x - mx) for x in lp]
    post = [x / math.fsum(w) for x in w]
    code = (d[0, 0] * 4 + d[0, 1] * 2 + d[0, 2]).astype(int)
    freq = np.bincount(code, minlength=8) / K
    for s, (p, f) in enumerate(zip(post, freq)):
        se = math.sqrt(p * (1.0 - p) / K)
        print(f"{kind} state {states[s]}: posterior {p:.5f}, frequency {f:.5f}, {abs(f - p) / se:.2f} se")
    for p, f in zip(post, freq):
        assert abs(f - p) <= 5.0 * math.sqrt(p * (1.0 - p) / K)


# ---- 6. stream hygiene: windows and a 1 + 3 chain split reproduce the single run bit for bit
def test_windows_and_chain_offset_bmg_mixed():
    d, V = cached("MIX", "bmg", 2, 4, 200, True, True)[:2]
    d2 = run("MIX", "bmg", 2, 4, 200, True, True, windows=[77, 123])[0]
    np.testing.assert_array_equal(d2, d)
    da = run("MIX", "bmg", 2, 1, 200, True, True, init=V[:1])[0]
    db = run("MIX", "bmg", 2, 3, 200, True, True, chain_offset=1, init=V[1:])[0]
    np.testing.assert_array_equal(np.concatenate([da, db], axis=2), d)


def test_windows_and_chain_offset_bia():
    d, V, _, _, t = run("S6", "bia", 1, 4, 200, tune=True)
    d2, _, _, _, t2 = run("S6", "bia", 1, 4, 200, windows=[77, 123], tune=True)
    np.testing.assert_array_equal(d2, d)
    np.testing.assert_array_equal(t2, t)
    da, _, _, _, ta = run("S6", "bia", 1, 1, 200, init=V[:1], tune=True)
    db, _, _, _, tb = run("S6", "bia", 1, 3, 200, chain_offset=1, init=V[1:], tune=True)
    np.testing.assert_array_equal(np.concatenate([da, db], axis=2), d)
    np.testing.assert_array_equal(np.concatenate([ta, tb], axis=0), t)


# ---- 7. kernel selection: the specialised kernel declines and names the sampler; the interpreter runs
@pytest.mark.parametrize("dn,kind,k,mixed", [("S6", "bmg", 3, False), ("S6", "bmc3", 3, False), ("S6", "bia", 1, False),
                                             ("MIX", "bmg", 2, True)])
def test_interpreter_vs_default(dn, kind, k, mixed, monkeypatch):
    d, V, (jit, info) = run(dn, kind, k, 4, 100, mixed)[:3]
    assert not jit and kind.upper() in info, info
    monkeypatch.setenv("MMB_IR_JIT", "0")
    d0, _, (jit0, info0) = run(dn, kind, k, 4, 100, mixed)[:3]
    assert not jit0 and "MMB_IR_JIT=0" in info0
    np.testing.assert_array_equal(d0, d)


# ---- 8. model statistics on a model with a binary block (the rule of test_gpu_dgs.test_logpdf_dic_predict)
def test_logpdf_dic_predict():
    mb = _mb()
    D = br.S6
    m, inputs, inits = br.model(mb.ir, D)
    m.setsamplers([mb.BMG("gamma", k=2)])
    K, n = 4, 50
    sim = mb.mcmc(m, inputs, inits(K), n, chains=K, seed=SEED, keep_device=True)
    assert sim.value.shape == (n, 6, K)
    lp = sim.logpdf(["gamma", "y"]).value
    worst = 0.0
    for i in range(n):
        for k in range(K):
            want, mag = br.logpdf_gamma_y(D, list(sim.value[i, :, k]))
            worst = max(worst, abs(lp[i, 0, k] - want) / mag)
            assert abs(lp[i, 0, k] - want) <= 1e-12 * mag
    print(f"logpdf: worst error {worst:.2e} of the sum of absolute terms")
    # the deviance at the posterior mean of a discrete node is undefined: refused, not garbage
    with pytest.raises(mb.ArgumentError, match="discrete node"):
        sim.dic()
    # predict(y): mu + z on the draw's own gamma, z = normal #e of the node's predict stream
    import oracle_lib
    L = oracle_lib.Oracle().L
    yh = sim.predict(["y"]).value
    nid = m.order.index("y")
    for i in (0, n - 1):
        for k in range(K):
            g = sim.value[i, :, k]
            for e in (0, 11, 24):
                z = L.orc_normal(SEED, k, sim.start + i * sim.thin, 256 + nid, 0, e)
                mu = D.X[0][e] * D.b0[0] * g[0]
                for j in range(1, 6):
                    mu = mu + D.X[j][e] * D.b0[j] * g[j]
                assert yh[i, e, k] == mu + 1.0 * z
