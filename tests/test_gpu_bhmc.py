"""BHMC blocks on the device against csrc/bhmc.h driven from the host (bit for bit, a flat density) and against the
plain-Python restatement (tests/bhmc_ref.py; decision-exact away from thresholds).  All runs: thin 1, burnin 0, every
sampled node monitored.

Position and velocity after each replayed update match the restatement to bhmc_ref.POS_TOL = 2.4e-11 of the
particle's size (bhmc_ref.row_gap): 100 times the 2.4e-13 that tests/test_bhmc.py measures between the restatement with
its log densities summed by math.fsum and summed naively in reversed order, the device's summation order being a
third one.
"""
import itertools
import math

import numpy as np
import pytest

import bhmc_ref as hr
import binary_ref as br

pytestmark = pytest.mark.gpu
SEED = hr.SEED
PI = math.pi


def _mb():
    import _mamba_path
    return _mamba_path.load()


def _normal():
    import oracle_lib
    return oracle_lib.Oracle().L.orc_normal


def build(dn, T, refresh, K, mixed=False, first=True):
    mb = _mb()
    m, inputs, inits = br.model(mb.ir, hr.DATA[dn], br.prior_of(dn), mixed)
    bl = [mb.BHMC("gamma", T, refresh=refresh)]
    ot = [mb.RWM("beta", 0.3), mb.Slice("s2", 1.0, transform=True)] if mixed else []
    m.setinputs(inputs).setsamplers(bl + ot if first else ot + bl)
    return m, m.init_matrix(hr.inits_of(dn, inits)(K), K)


def flat(n, T, K):
    mb = _mb()
    m = mb.ir.Model(gamma=mb.ir.Stochastic(1, lambda: mb.ir.Bernoulli(0.5)))
    m.setsamplers([mb.BHMC("gamma", T)])
    return m, m.init_matrix([{"gamma": [float((k >> (j % 5)) & 1) for j in range(n)]} for k in range(K)], K)


def stepped(m, V, iters, chain_offset=0):
    """One iteration per window: (draws [iters, pmon, K], tune rows before the first and after every iteration, stats)."""
    eng = _mb().Engine(m)
    eng.init_chains(V, chain_offset=chain_offset, seed=SEED)
    tunes, draws = [eng.tune().copy()], []
    for _ in range(iters):
        draws.append(eng.run(1))
        tunes.append(eng.tune().copy())
    out = np.concatenate(draws, axis=0), tunes, eng.accept_stats(), eng.bhmc_stats()
    eng.close()
    return out


def run(m, V, windows, chain_offset=0):
    eng = _mb().Engine(m)
    eng.init_chains(V, chain_offset=chain_offset, seed=SEED)
    d = np.concatenate([eng.run(w) for w in windows], axis=0)
    t = eng.tune().copy()
    eng.close()
    return d, t


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return hr.host_lib(tmp_path_factory.mktemp("bhmc_host"))


# ---- 1. a flat density: the device's rows equal the host's drive of csrc/bhmc.h bit for bit
@pytest.mark.parametrize("n,Tpi", [(1, 2.5), (3, 2.5), (3, 6.5), (32, 2.5)])
def test_flat_density_bit_for_bit(host, n, Tpi):
    """Bernoulli(0.5) with no targets, 5 chains (a half-filled wave), six iterations, one per window: after every window
    the tune rows equal a host replay that drives bhmc.h's per-element functions on the same MMB_SUB_INIT normals (the
    log-density difference is an exact 0 on both sides); value = position > 0; wallhits == wallcrosses == the sign changes
    of the closed-form rotation."""
    K, iters, T = 5, 6, Tpi * PI
    m, V = flat(n, T, K)
    d, tunes, stats, bst = stepped(m, V, iters)
    assert tunes[0].shape == (K, 2 * n + 3) and not tunes[0].any()
    z, ops = _normal(), hr.HostOps(host)
    for c in range(K):
        row = [0.0] * (2 * n + 3)
        for t in range(iters):
            o = hr.bhmc_step(lambda x: n * math.log(0.5), n, row, T, False,
                             lambda k: z(SEED, c, t + 1, 0, hr.SUB_INIT, k), None, hr.BDec(), ops)
            assert o.done
            row = o.row
            np.testing.assert_array_equal(tunes[t + 1][c], np.array(row))
            np.testing.assert_array_equal(d[t, :, c], np.array(row[:n]) > 0.0)
        b0 = [z(SEED, c, 1, 0, hr.SUB_INIT, i) for i in range(n)]
        a0 = [z(SEED, c, 1, 0, hr.SUB_INIT, 32 + i) for i in range(n)]
        count = sum(hr.sign_changes(b, a, iters * T) for a, b in zip(a0, b0))
        assert tunes[-1][c][2 * n] == tunes[-1][c][2 * n + 1] == count
    assert stats[0]["updates"] == stats[0]["accepts"] == K * iters
    np.testing.assert_array_equal(bst[0]["wallhits"], tunes[-1][:, 2 * n])


# ---- 2. replay against the restatement, every update from the device's own pre-update row
@pytest.mark.parametrize("refresh", [False, True], ids=["reference", "refresh"])
@pytest.mark.parametrize("dn,Tpi,mixed,first", hr.REPLAY_CASES,
                         ids=[f"{c[0]}{'' if c[3] else '-last'}" for c in hr.REPLAY_CASES])
def test_replay(dn, Tpi, mixed, first, refresh):
    """8 chains, 25 iterations: no mismatch, at most 2 threshold skips, updates == chains x iterations, and position and
    velocity within POS_TOL = 2.4e-11 (100 times the measured summation gap 2.4e-13, see the module's docstring).  EDGE:
    -Inf and NaN log-density differences; a crossing at infinite speed stalls the update, a NaN reflects."""
    K, iters, T = hr.K_REPLAY, hr.ITERS_REPLAY, Tpi * PI
    m, V = build(dn, T, refresh, K, mixed, first)
    d, tunes, stats, _ = stepped(m, V, iters)
    sp = hr.spec(dn, mixed, first)
    R = hr.Replay(_normal(), sp, SEED, T, refresh).run(V, d, [[list(r) for r in t] for t in tunes])
    print(f"{dn} T={Tpi} pi refresh={refresh}: {R.updates} updates, {R.events} events, {R.stalls} stalls {R.why}, "
          f"{R.infspeed} crossings at infinite speed, {R.skips} skips, {len(R.mismatch)} mismatches, gap {R.gap:.3e}")
    assert R.mismatch == []
    assert R.skips <= 2
    assert R.updates == K * iters
    assert R.gap <= hr.POS_TOL
    assert set(np.unique(d[:, :hr.DATA[dn].n, :])) <= {0.0, 1.0}
    b = R.b
    assert stats[b]["updates"] == K * iters and stats[b]["accepts"] == R.done
    if dn == "EDGE":
        assert R.stalls > 0 and R.infspeed > 0
    else:
        assert R.stalls == 0 and R.events > 0
    if mixed:
        assert len(np.unique(d[:, 3:6, :])) > 20 and len(np.unique(d[:, 6, :])) > 20  # beta and s2 move


# ---- 3. windows and a 1 + 3 chain split reproduce the single run bit for bit, tune rows included
@pytest.mark.parametrize("refresh", [False, True], ids=["reference", "refresh"])
def test_windows_and_chain_offset(refresh):
    T = 2.5 * PI
    m, V = build("MIX", T, refresh, 4, True, True)
    d, t = run(m, V, [20])
    d2, t2 = run(m, V, [7, 13])
    np.testing.assert_array_equal(d2, d)
    np.testing.assert_array_equal(t2, t)
    ma, _ = build("MIX", T, refresh, 1, True, True)
    da, ta = run(ma, V[:1], [20])
    mb3, _ = build("MIX", T, refresh, 3, True, True)
    db, tb = run(mb3, V[1:], [20], chain_offset=1)
    np.testing.assert_array_equal(np.concatenate([da, db], axis=2), d)
    np.testing.assert_array_equal(np.concatenate([ta, tb], axis=0), t)
    assert t[:, -1].all() and (t[:, -3] > 0).all()


# ---- 4. tune rows: set then get is exact; a run continued from saved rows equals the uninterrupted one
def test_tune_rows_round_trip_and_continue():
    T, n = 12.5 * PI, 6
    m, V = build("S6", T, False, 4)
    d, t = run(m, V, [10])
    eng = _mb().Engine(m)
    eng.init_chains(V, seed=SEED)
    d1 = eng.run(4)
    saved = eng.tune().copy()
    changed = saved.copy()
    changed[:, :2 * n] = 0.5 - 0.25 * changed[:, :2 * n]
    changed[:, 2 * n] += 2.0 ** 33  # the counters are not 32-bit
    changed[:, 2 * n + 1] = 7.0
    changed[1, 2 * n + 2] = 0.0
    eng.set_tune(changed)
    np.testing.assert_array_equal(eng.tune(), changed)
    eng.set_tune(saved)
    d2 = eng.run(6)
    np.testing.assert_array_equal(np.concatenate([d1, d2], axis=0), d)
    np.testing.assert_array_equal(eng.tune(), t)
    bad = saved.copy()
    bad[0, 2 * n] = -1.0
    with pytest.raises(Exception, match="BHMC tune row"):
        eng.set_tune(bad)
    eng.close()


# ---- 5. stalls, reached through set_tune only: a handled condition
def test_stalls_leave_the_chain_as_it_was():
    """Chain 1 gets position_0 = 0 with velocity_0 > 0 (a zero move time, the reference's error), chain 2 (in one wave
    with the healthy chain 3) a NaN position: after one iteration their values and rows are unchanged, the others
    moved, and accept_stats shows 4 updates, 2 accepts."""
    T, n, K = 2.5 * PI, 3, 4
    m, V = build("S3", T, False, K)
    eng = _mb().Engine(m)
    eng.init_chains(V, seed=SEED)
    rows = eng.tune().copy()
    rng = np.random.RandomState(3)
    rows[:, :2 * n] = rng.standard_normal((K, 2 * n))
    rows[:, 2 * n:] = [5.0, 3.0, 1.0]
    rows[1, 0], rows[1, n] = 0.0, 0.7
    rows[2, 1] = math.nan
    eng.set_tune(rows)
    d = eng.run(1)
    after = eng.tune()
    stats = eng.accept_stats()
    eng.close()
    for c in (1, 2):
        np.testing.assert_array_equal(after[c], rows[c])
        np.testing.assert_array_equal(d[0, :, c], V[c])
    for c in (0, 3):
        assert not np.array_equal(after[c][:2 * n], rows[c][:2 * n]) and after[c][2 * n] > 5.0
        np.testing.assert_array_equal(d[0, :, c], after[c][:n] > 0.0)
    assert (stats[0]["updates"], stats[0]["accepts"]) == (4, 2)


# ---- 6. the exact posterior, refresh=True only
def test_exact_posterior_with_refresh():
    """S3's three coupled indicators, 4096 independent chains, T = 3.5 pi, the 40th draw of each: all 8 state frequencies
    within 5 standard errors sqrt(p (1 - p) / 4096) of the enumerated posterior.  refresh=False, the reference, does not
    target the posterior (its velocity is never redrawn) and is not tested against it."""
    K = 4096
    m, V = build("S3", 3.5 * PI, True, K)
    eng = _mb().Engine(m)
    eng.init_chains(V, seed=SEED)
    d = eng.run(40, burnin=39)
    stats = eng.accept_stats()
    eng.close()
    assert d.shape == (1, 3, K) and stats[0]["updates"] == stats[0]["accepts"] == 40 * K
    states = list(itertools.product([0.0, 1.0], repeat=3))
    lp = [br.logpdf_gamma_y(br.S3, list(g))[0] for g in states]
    w = [math.exp(x - max(lp)) for x in lp]
    post = [x / math.fsum(w) for x in w]
    code = (d[0, 0] * 4 + d[0, 1] * 2 + d[0, 2]).astype(int)
    freq = np.bincount(code, minlength=8) / K
    for s, (p, f) in enumerate(zip(post, freq)):
        print(f"state {states[s]}: posterior {p:.5f}, frequency {f:.5f}, {abs(f - p) / math.sqrt(p * (1 - p) / K):.2f} se")
    for p, f in zip(post, freq):
        assert abs(f - p) <= 5.0 * math.sqrt(p * (1.0 - p) / K)


# ---- 7. kernel selection, the statistics and logpdf on the sampled node
def test_decline_by_name_stats_and_logpdf():
    mb = _mb()
    n, K, iters = 6, 4, 30
    m, V = build("S6", 12.5 * PI, False, K)
    eng = mb.Engine(m)
    eng.init_chains(V, seed=SEED)
    eng.run(iters)
    jit, info = eng.ir_jit()
    t, bst = eng.tune(), eng.bhmc_stats()
    eng.close()
    assert not jit and "BHMC" in info, info
    assert list(bst) == [0]
    np.testing.assert_array_equal(bst[0]["wallhits"], t[:, 2 * n])
    np.testing.assert_array_equal(bst[0]["wallcrosses"], t[:, 2 * n + 1])
    assert (bst[0]["wallhits"] >= bst[0]["wallcrosses"]).all() and (bst[0]["wallcrosses"] > 0).all()
    assert (bst[0]["wallhits"] <= iters * hr.event_bound(n, 12.5 * PI)).all()
    m2, inputs, inits = br.model(mb.ir, br.S6)
    m2.setsamplers([mb.BHMC("gamma", 12.5 * PI)])
    sim = mb.mcmc(m2, inputs, inits(K), iters, chains=K, seed=SEED, keep_device=True)
    assert sim.value.shape == (iters, n, K)
    lp = sim.logpdf(["gamma", "y"]).value
    for i in range(iters):
        for k in range(K):
            want, mag = br.logpdf_gamma_y(br.S6, list(sim.value[i, :, k]))
            assert abs(lp[i, 0, k] - want) <= 1e-12 * mag
    with pytest.raises(mb.ArgumentError, match="discrete node"):
        sim.dic()
