"""Lazy AMM factor store of the 32-lane sweep kernels (samplers.h amm, two moment buffers).

Within a launch a full-rank adaptive update keeps its factor in registers only when the next
update of the block runs in the same launch and adapts: the next proposal is the carried one and
the next full-rank update replaces the factor.  The moments after m updates live in the buffer of
m's parity, so a chain whose NEXT update turns out rank deficient (amm.jl:88-90 keeps the older
SigmaLm) rebuilds the covariance of the update before from the other buffer, factorizes it again
and stores that factor.  None of this may be visible: draws, values and every tune field (Mv, Mvv,
factor, pivots, flags) equal the oracle's bit for bit at every launch boundary, whatever the
launch widths are, across a checkpoint, with adaptation ending inside a launch and with or without
the wavefront pairing of chains."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def rats(mamba, scheme=None):
    m = mamba.rats()
    m.setinputs(mamba.model.RATS_DATA)
    return m.setsamplers(scheme if scheme is not None else mamba.model.rats_scheme_gibbs_amm())


def amm_slices(mamba, m):
    """Per AMM block: (block index, offset in the tune row, d)."""
    out, off = [], 0
    for b, s in enumerate(m.samplers):
        d = m.block_dim(s)
        if s.kind == mamba.abi.MMB_SAMPLER_AMM:
            out.append((b, off, d))
            off += 4 + 2 * d + d * (d + 1)
        elif s.kind == mamba.abi.MMB_SAMPLER_AMWG:
            off += 2 + 2 * d
    return out


def assert_state(eng, st):
    np.testing.assert_array_equal(eng.values(), st["values"])
    np.testing.assert_array_equal(eng.tune(), st["tune"][:, :st["tl"]])


# ------------------------------------------------------------------ launch widths
W_K, W_SEED, W_BURNIN, W_THIN = 37, 29, 10, 3   # 37 chains: the last wavefront holds one chain
W_WINDOWS = (77, 73)


@pytest.fixture(scope="module")
def widths_oracle(mamba, oracle):
    """150 iterations from rats_init_ls as windows of 77 and 73: (draws, values, tune) after each."""
    m = rats(mamba)
    init = mamba.model.rats_init_ls(W_K, seed=4)
    st = oracle.new_state(m, init)
    ref = []
    for n in W_WINDOWS:
        d = oracle.run(m, st, n, burnin=W_BURNIN, thin=W_THIN, seed=W_SEED, nthreads=8)
        ref.append((d, st["values"].copy(), st["tune"][:, :st["tl"]].copy()))
    return m, init, ref


@pytest.mark.parametrize("width", [1, 3, 20])
def test_launch_widths(mamba, widths_oracle, monkeypatch, width):
    """Launches of 1 iteration (every update is a launch's last: nothing is lazy), 3 and 20 (the
    default; 77 = 3 x 20 + 17, 73 = 3 x 20 + 13).  After each window the draws, the values and the
    whole tune rows equal the oracle's; a checkpoint of values, tune and iteration taken after the
    first window, restored into a fresh engine, reaches the same bits after the second."""
    m, init, ref = widths_oracle
    monkeypatch.setenv("MMB_ITERS_PER_LAUNCH", str(width))
    eng = mamba.Engine(m)
    eng.init_chains(init, seed=W_SEED)
    ck = None
    for w, (n, (d, v, t)) in enumerate(zip(W_WINDOWS, ref)):
        np.testing.assert_array_equal(eng.run(n, burnin=W_BURNIN, thin=W_THIN), d)
        np.testing.assert_array_equal(eng.values(), v)
        np.testing.assert_array_equal(eng.tune(), t)
        if w == 0:
            ck = (eng.values(), eng.tune(), eng.iter)
    eng.close()
    # both classes are present, so full-rank updates were skipped and stored
    for b, off, dd in amm_slices(mamba, m):
        assert 0 < (ref[1][2][:, off + 2] != 0).sum() < W_K
    e2 = mamba.Engine(m)
    e2.init_chains(init, seed=W_SEED)
    e2.set_values(ck[0])
    e2.set_tune(ck[1])
    e2.set_iter(ck[2])
    np.testing.assert_array_equal(e2.tune(), ck[1])
    d, v, t = ref[1]
    np.testing.assert_array_equal(e2.run(W_WINDOWS[1], burnin=W_BURNIN, thin=W_THIN), d)
    np.testing.assert_array_equal(e2.values(), v)
    np.testing.assert_array_equal(e2.tune(), t)
    e2.close()


# ------------------------------------------------------------------ recovery path
# Chains started by set_tune with m = 100, Mv = the chain's alpha / beta and
# Mvv = Mv Mv' + EPS diag(Mv_i^2): Sigma = cc (Mvv - Mv Mv') is then EPS Mv_i^2 on the diagonal plus
# the rounding of the products (2^-53 relative), so with EPS = 2^-48 the rank test of the first
# updates is decided by rounding.  EPS and the seed were found with the oracle on the CPU (EPS
# 2^-52 .. 2^-50: a quarter of the updates full rank and few transitions; 2^-46 and above: all full
# rank; 2^-48: 70-75 % full rank); at seed 5 the 64 chains show 204 full -> deficient transitions
# in 40 iterations that are not at a launch's last iteration, chain 62 alone 8, chains 31..33 15.
R_EPS = 2.0 ** -48
R_SEED = 5
R_M0 = 100
R_ITERS = 40
R_WIDTH = 20
R_CASES = {64: 0, 1: 62, 3: 31}  # chains -> first chain of the 64


def craft(tune, init, slices):
    for c in range(tune.shape[0]):
        for (b, off, d), cols in zip(slices, (slice(1, 31), slice(33, 63))):
            T = d * (d + 1) // 2
            t = tune[c, off:off + 4 + 2 * d + 2 * T]
            t[:] = 0.0
            t[0], t[1] = 1.0, float(R_M0)
            mv = init[c, cols].copy()
            t[4:4 + d] = mv
            for i in range(d):
                for k in range(i + 1):
                    v = mv[i] * mv[k]
                    t[4 + d + i * (i + 1) // 2 + k] = v + R_EPS * v if i == k else v
            t[4 + 2 * d + 2 * T - d:4 + 2 * d + 2 * T] = np.arange(d)


@pytest.fixture(scope="module")
def recovery_oracle(mamba, oracle):
    """The oracle on the 64 crafted chains, one chain and one iteration at a time: per chain the
    draws, the final values and tune row, and whether each block's update was full rank."""
    m = rats(mamba)
    sl = amm_slices(mamba, m)
    init = mamba.model.rats_init_ls(64, seed=R_SEED)
    pmon = len(m.monitor_names)
    draws = np.zeros((R_ITERS, pmon, 64), order="F")
    full = np.zeros((R_ITERS + 1, 64, len(sl)), dtype=bool)
    rank_sum = np.zeros((64, len(sl)), dtype=np.int64)
    values, tune = [], []
    for c in range(64):
        st = oracle.new_state(m, init[c:c + 1])
        craft(st["tune"], init[c:c + 1], sl)
        for t in range(1, R_ITERS + 1):
            oracle.amm_stats(reset=True)
            draws[t - 1, :, c] = oracle.run(m, st, 1, burnin=0, thin=1, seed=R_SEED, chain_offset=c)[0, :, 0]
            so = oracle.amm_stats(reset=True)
            for j, (b, off, d) in enumerate(sl):
                assert so[b]["updates"] == 1
                full[t, c, j] = so[b]["full_rank"] == 1
                rank_sum[c, j] += so[b]["rank_sum"]
        values.append(st["values"][0].copy())
        tune.append(st["tune"][0, :st["tl"]].copy())
    return m, sl, init, draws, np.array(values), np.array(tune), full, rank_sum


def transitions(full, c0, K):
    """Updates of chains c0 .. c0 + K - 1 that were full rank at t and are deficient at t + 1, t not
    a launch's last iteration at R_WIDTH (there the factor is stored anyway)."""
    return sum(int((full[t, c0:c0 + K] & ~full[t + 1, c0:c0 + K]).sum())
               for t in range(1, R_ITERS) if t % R_WIDTH != 0)


@pytest.mark.parametrize("K", [64, 1, 3])
def test_recovery_path(mamba, recovery_oracle, monkeypatch, K):
    """A marked chain's next update is rank deficient: the factor of the update before has to come
    back exactly.  64 chains (wavefronts that pair a recovering chain with one that is not), one
    chain (the upper lane group absent) and three (the last wavefront holds one chain)."""
    m, sl, init64, draws, values, tune, full, rank_sum = recovery_oracle
    c0 = R_CASES[K]
    assert transitions(full, c0, K) >= 8, transitions(full, c0, K)
    monkeypatch.setenv("MMB_ITERS_PER_LAUNCH", str(R_WIDTH))
    eng = mamba.Engine(m)
    eng.init_chains(init64[c0:c0 + K], chain_offset=c0, seed=R_SEED)
    t0 = eng.tune()
    craft(t0, init64[c0:c0 + K], sl)
    eng.set_tune(t0)
    dg = eng.run(R_ITERS, burnin=0, thin=1)
    np.testing.assert_array_equal(dg, draws[:, :, c0:c0 + K])
    np.testing.assert_array_equal(eng.values(), values[c0:c0 + K])
    np.testing.assert_array_equal(eng.tune(), tune[c0:c0 + K])
    sg = eng.amm_stats()
    for j, (b, off, d) in enumerate(sl):
        assert sg[b]["updates"] == K * R_ITERS
        assert sg[b]["full_rank"] == int(full[1:, c0:c0 + K, j].sum())
        assert sg[b]["rank_sum"] == int(rank_sum[c0:c0 + K, j].sum())
    eng.close()


def test_chain_order_on_and_off(mamba, recovery_oracle, monkeypatch):
    """The crafted chains as two windows of 20 with a fresh pairing table before the second
    (MMB_ORDER_EVERY=1), and in identity order (MMB_ORDER_CHAINS=0): the same bits, the oracle's."""
    m, sl, init64, draws, values, tune, full, rank_sum = recovery_oracle
    monkeypatch.setenv("MMB_ITERS_PER_LAUNCH", str(R_WIDTH))
    monkeypatch.setenv("MMB_ORDER_EVERY", "1")
    orders = {}
    for mode in ("ordered", "identity"):
        if mode == "identity":
            monkeypatch.setenv("MMB_ORDER_CHAINS", "0")
        eng = mamba.Engine(m)
        eng.init_chains(init64, seed=R_SEED)
        t0 = eng.tune()
        craft(t0, init64, sl)
        eng.set_tune(t0)
        a = eng.run(R_ITERS // 2, burnin=0, thin=1)
        orders[mode] = eng.chain_order().copy()
        b = eng.run(R_ITERS - R_ITERS // 2, burnin=0, thin=1)
        np.testing.assert_array_equal(np.concatenate([a, b]), draws)
        np.testing.assert_array_equal(eng.values(), values)
        np.testing.assert_array_equal(eng.tune(), tune)
        eng.close()
    np.testing.assert_array_equal(orders["identity"], np.arange(64))
    assert (orders["ordered"] != np.arange(64)).any()  # the second window ran permuted


# ------------------------------------------------------------------ adapt = burnin
def test_adaptation_ends_inside_a_launch(mamba, oracle, monkeypatch):
    """adapt="burnin" with the model's burn-in at iteration 107, the 7th of the launch 101..120: the
    update at 107 is the block's last adaptive one, so its factor is stored although the launch
    goes on, and the proposals from 108 on read it.  Parity with the oracle, and valid factors in
    the tune rows afterwards."""
    sch = mamba.model.rats_scheme_gibbs_amm()
    sch[1] = mamba.AMM("alpha", np.eye(30), adapt="burnin")
    sch[4] = mamba.AMM("beta", 0.01 * np.eye(30), adapt="burnin")
    m = rats(mamba, sch)
    init = mamba.model.rats_init_ls(48, seed=8)
    monkeypatch.setenv("MMB_ITERS_PER_LAUNCH", "20")
    eng = mamba.Engine(m)
    eng.init_chains(init, seed=13)
    dg = eng.run(130, burnin=4, thin=2, model_burnin=107)
    st = oracle.new_state(m, init)
    do = oracle.run(m, st, 130, burnin=4, thin=2, seed=13, model_burnin=107, nthreads=8)
    np.testing.assert_array_equal(dg, do)
    assert_state(eng, st)
    t = eng.tune()
    for b, off, d in amm_slices(mamba, m):
        assert (t[:, off + 1] == 107).all() and (t[:, off] == 0).all()
        assert (t[:, off + 2] == 1).sum() >= 8  # chains that propose from a stored factor
    eng.close()
