"""Chain parts of the fused sweep (engine.cpp mmb_run, MMB_SWEEP_PARTS): the workgroups of a
window are dealt round-robin to P parts, each a sequence of sweep launches on its own stream,
joined on the engine stream at the window's end.  Every chain keeps its own state, tune rows,
draws column and Philox id, so draws, values, tune and the AMM counters equal the one-part run
and the oracle bit for bit, for every P and for shapes whose workgroup count is no multiple of
P (K = 600: 75 workgroups), whose last workgroup is ragged (K = 52) and that leave parts empty
(K = 8: one workgroup).

Each run is two windows of 45 and 35 iterations at 20 iterations per launch (three launches of
15 per part, then 18 + 17), thin 3 behind a burnin of 6, with a fresh slot -> chain table after
every window (MMB_ORDER_EVERY=1), so the second window runs permuted.  mmb_kernel_time counts
every non-empty part's launches and reports the time during which at least one of them was in
flight, which cannot exceed the window's wall time."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WINDOWS = (45, 35)
LAUNCHES = (3, 2)  # per part, at 20 iterations per launch
BURNIN, THIN = 6, 3
CPW = 8            # chains per workgroup of the rats kernels


def rats(mamba, scheme):
    m = mamba.rats()
    m.setinputs(mamba.model.RATS_DATA)
    return m.setsamplers(scheme)


def run_parts(mamba, m, init, seed, parts, monkeypatch):
    monkeypatch.setenv("MMB_ORDER_EVERY", "1")
    monkeypatch.setenv("MMB_ITERS_PER_LAUNCH", "20")
    monkeypatch.setenv("MMB_SWEEP_PARTS", str(parts))
    eng = mamba.Engine(m)
    eng.init_chains(init, seed=seed)
    eng.sync()
    draws, timing = [], []
    for iters in WINDOWS:
        t0 = time.perf_counter()
        d = eng.run(iters, burnin=BURNIN, thin=THIN, time_kernels=True)
        eng.sync()
        wall_ms = (time.perf_counter() - t0) * 1e3
        kms, launches, units = eng.kernel_time()
        draws.append(d)
        timing.append((kms, launches, units, wall_ms))
    out = (np.concatenate(draws), eng.values(), eng.tune(), eng.amm_stats(), timing)
    eng.close()
    return out


@pytest.fixture(scope="module")
def gibbs_amm_oracle(mamba, oracle):
    """The oracle's run of the largest shape, once: chains are independent and keep their ids, so
    the smaller shapes are its leading chains."""
    m = rats(mamba, mamba.model.rats_scheme_gibbs_amm())
    init = mamba.model.rats_init_ls(16384, seed=1000)[:600]
    st = oracle.new_state(m, init)
    do = oracle.run(m, st, sum(WINDOWS), burnin=BURNIN, thin=THIN, seed=33, nthreads=8)
    return m, init, do, st["values"].copy(), st["tune"][:, :st["tl"]].copy()


@pytest.mark.parametrize("K", [600, 52, 8])
def test_parts_equal_one_part_and_oracle(mamba, oracle, gibbs_amm_oracle, monkeypatch, K):
    m, init_all, do, vo, to = gibbs_amm_oracle
    init = init_all[:K]
    nwg = (K + CPW - 1) // CPW
    out = {p: run_parts(mamba, m, init, 33, p, monkeypatch) for p in (1, 2, 3, 4)}
    d1, v1, t1, s1, _ = out[1]
    np.testing.assert_array_equal(d1, do[:, :, :K])
    np.testing.assert_array_equal(v1, vo[:K])
    np.testing.assert_array_equal(t1, to[:K])
    if K == 600:  # the classes split, so the second window's table is not the identity
        assert 0.2 < (t1[:, 2] != 0).mean() < 0.9
    for p in (1, 2, 3, 4):
        d, v, t, s, timing = out[p]
        np.testing.assert_array_equal(d, d1)
        np.testing.assert_array_equal(v, v1)
        np.testing.assert_array_equal(t, t1)
        assert sorted(s) == sorted(s1) and s
        for b in s:
            for f in ("updates", "full_rank", "rank_sum"):
                assert s[b][f] == s1[b][f], (p, b, f)
            assert s[b]["updates"] == K * sum(WINDOWS)
        live = min(p, nwg)  # parts past the last workgroup launch nothing and are not counted
        for (kms, launches, units, wall_ms), iters, per_part in zip(timing, WINDOWS, LAUNCHES):
            print(f"K={K} P={p} window={iters}: kernel {kms:.3f} ms, wall {wall_ms:.3f} ms, launches {launches}")
            assert launches == live * per_part, (p, iters, launches)
            assert units == iters * K
            assert 0.0 < kms <= wall_ms, (p, iters, kms, wall_ms)


def test_parts_slice_overflow_read_after_join(mamba, oracle, monkeypatch):
    """The reference Slice + AMWG scheme at two parts: mmb_run reads the Slice overflow counter on
    the engine stream after the join, and the results equal the one-part run and the oracle."""
    m = rats(mamba, mamba.model.rats_scheme_reference())
    init = mamba.model.rats_init_matrix(100)
    one = run_parts(mamba, m, init, 71, 1, monkeypatch)
    two = run_parts(mamba, m, init, 71, 2, monkeypatch)
    st = oracle.new_state(m, init)
    do = oracle.run(m, st, sum(WINDOWS), burnin=BURNIN, thin=THIN, seed=71, nthreads=8)
    for x in (one, two):
        np.testing.assert_array_equal(x[0], do)
        np.testing.assert_array_equal(x[1], st["values"])
        np.testing.assert_array_equal(x[2], st["tune"][:, :st["tl"]])
    for (kms, launches, units, wall_ms), per_part in zip(two[4], LAUNCHES):
        assert launches == 2 * per_part
        assert 0.0 < kms <= wall_ms
