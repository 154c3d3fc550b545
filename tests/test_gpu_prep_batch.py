"""The rats vector blocks' per-chain scalar constants from one lane-parallel pass (models.h
prep_pass, sweep.h).

A 30-d block update (AMM, AMWG) needs the prior sd and log sd of its node and y's ScalMat
constants: functions of s2_alpha or s2_beta and of s2_c alone.  One pass forms all of them, a
variance node per lane, and keeps them in the chain's LDS region; a wave-uniform stale bit per
variance node -- all set at a launch's start, one set after every block whose descriptor holds
that node -- decides whether a vector block runs the pass or reads what is there.  The oracle
knows no pass and forms the constants inside every block's logpdf!, so draws, values and the
full tune rows equal to it bit for bit mean that no block ever read a constant of an older
variance: whatever the block order, across launch boundaries (nothing is carried over one) and
after a host write of the values.
"""
import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu

S2_C, MU_ALPHA, S2_ALPHA, MU_BETA, S2_BETA = 0, 31, 32, 63, 64  # columns of the values matrix


def rats(mamba, scheme):
    m = mamba.rats()
    m.setinputs(mamba.model.RATS_DATA)
    return m.setsamplers(scheme)


def scheme(mamba, name):
    G, AMM = mamba.Gibbs, mamba.AMM
    if name in ("gibbs_amm", "reference"):
        return bench.scheme_for(mamba, name)
    if name == "amm_consecutive":  # beta's update finds everything fresh: it reuses alpha's pass
        return [G("s2_c"), AMM("alpha", np.eye(30)), AMM("beta", 0.01 * np.eye(30)), G("mu_alpha"),
                G("s2_alpha"), G("mu_beta"), G("s2_beta")]
    if name == "s2c_between":  # s2_c is written between the two: beta's update runs the pass again
        return [AMM("alpha", np.eye(30)), G("s2_c"), AMM("beta", 0.01 * np.eye(30)), G("mu_alpha"),
                G("s2_alpha"), G("mu_beta"), G("s2_beta")]
    if name == "gibbs_only_plus_amm":
        return bench.scheme_for(mamba, "gibbs_only") + [AMM("beta", 0.01 * np.eye(30))]
    raise ValueError(name)


SCHEMES = ["gibbs_amm", "reference", "amm_consecutive", "s2c_between", "gibbs_only_plus_amm"]
ITERS, PER_LAUNCH, BURNIN, THIN, SEED = 9, 4, 2, 1, 23  # launches of 4, 4 and 1 iterations


def gpu_windows(mamba, m, init, windows, edit=None):
    """Runs the windows (iterations each) on one engine; edit(values) -> values is applied through
    the values setter between them.  Returns draws, values, tune rows."""
    eng = mamba.Engine(m)
    eng.init_chains(init, seed=SEED)
    draws = []
    for i, iters in enumerate(windows):
        if i and edit is not None:
            eng.set_values(edit(eng.values()))
        draws.append(eng.run(iters, burnin=BURNIN, thin=THIN))
    out = np.concatenate([d for d in draws if d is not None]), eng.values(), eng.tune()
    eng.close()
    return out


def oracle_windows(oracle, m, init, windows, edit=None):
    st = oracle.new_state(m, init)
    draws = []
    for i, iters in enumerate(windows):
        if i and edit is not None:
            st["values"][...] = edit(st["values"].copy())
        draws.append(oracle.run(m, st, iters, burnin=BURNIN, thin=THIN, seed=SEED, nthreads=8))
    return np.concatenate([d for d in draws if d is not None]), st["values"], st["tune"][:, :st["tl"]]


def assert_same_bits(gpu, ref):
    """Bit for bit wherever the reference is a number; NaN where it is NaN (a NaN's sign and
    payload are the processor's choice, as in test_gpu_adversarial)."""
    for x, y in zip(gpu, ref):
        assert x.shape == y.shape
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        nan = np.isnan(y)
        np.testing.assert_array_equal(np.isnan(x), nan)
        np.testing.assert_array_equal(np.where(nan, 0, x.view(np.uint64)), np.where(nan, 0, y.view(np.uint64)))


@pytest.mark.parametrize("chains", [2, 3, 66])
@pytest.mark.parametrize("name", SCHEMES)
def test_schemes(mamba, oracle, monkeypatch, name, chains):
    """2 chains (one wave), 3 (the last wave's upper lane group is empty) and 66 (two workgroups,
    the last one a single wave); 9 iterations at 4 per launch, so every launch starts stale and
    the last one is ragged.  gibbs_amm: one pass per iteration, at alpha's update; reference:
    AMWG's amwg_terms / amwg_dm read the same constants, Slice writes the variances; the two
    reordered schemes and gibbs_only plus one AMM block: see scheme()."""
    monkeypatch.setenv("MMB_ITERS_PER_LAUNCH", str(PER_LAUNCH))
    m = rats(mamba, scheme(mamba, name))
    init = mamba.model.rats_init_ls(chains, seed=11)
    ref = oracle_windows(oracle, m, init, [ITERS])
    assert not np.isnan(ref[0]).any() and not np.isnan(ref[1]).any()
    assert_same_bits(gpu_windows(mamba, m, init, [ITERS]), ref)


def test_values_setter_between_windows(mamba, oracle, monkeypatch):
    """s2_c, s2_alpha and s2_beta overwritten through the values setter between two windows of 5
    iterations (launches of 4 and 1): the second window equals an oracle continued from the
    same edited state.  s2c_between reads s2_c in alpha's update before any block writes it, so
    the value used there is the host's."""
    monkeypatch.setenv("MMB_ITERS_PER_LAUNCH", str(PER_LAUNCH))

    def edit(v):
        k = np.arange(v.shape[0])
        v[:, S2_C] = 20.0 + 0.5 * k
        v[:, S2_ALPHA] = 3.0 + 0.25 * k
        v[:, S2_BETA] = 0.125 + 0.015625 * k
        return v

    for name in ("gibbs_amm", "s2c_between"):
        m = rats(mamba, scheme(mamba, name))
        init = mamba.model.rats_init_ls(66, seed=12)
        ref = oracle_windows(oracle, m, init, [5, 5], edit)
        assert_same_bits(gpu_windows(mamba, m, init, [5, 5], edit), ref)


def test_zero_variance(mamba, oracle, monkeypatch):
    """A variance of 0.0: sd 0, log sd -inf, 1 / value +inf, yk -inf, formed by the pass with the
    operations the oracle applies.  s2c_between reads the initial s2_c in alpha's first update;
    chain 1 starts with s2_c = 0 (alpha's first proposal meets a non-finite logpdf! and is
    rejected, then Gibbs redraws s2_c and the chain goes on in numbers), chain 2 with s2_alpha = 0
    and chain 3 with s2_beta = 0 (the conjugate draws of the mean and the variance turn NaN and
    stay NaN); chains 0 and 4 are ordinary.  Neither side raises an error for such a state: both
    give the same bits where the oracle has numbers and NaN where it has NaN."""
    monkeypatch.setenv("MMB_ITERS_PER_LAUNCH", str(PER_LAUNCH))
    m = rats(mamba, scheme(mamba, "s2c_between"))
    init = mamba.model.rats_init_ls(5, seed=13)
    init[1, S2_C] = 0.0
    init[2, S2_ALPHA] = 0.0
    init[3, S2_BETA] = 0.0
    ref = oracle_windows(oracle, m, init, [ITERS])
    assert np.isfinite(ref[1][[0, 1, 4]]).all()  # the s2_c = 0 chain recovers
    assert np.isnan(ref[1][2, MU_ALPHA]) and np.isnan(ref[1][3, MU_BETA])
    assert_same_bits(gpu_windows(mamba, m, init, [ITERS]), ref)
