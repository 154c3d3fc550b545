"""Batched state-independent draws of the 32-lane sweep kernels (samplers.h predraw, sweep.h).

One pass draws the Gibbs variates and AMM accept uniforms of Q = max(1, 32 / nb) consecutive
iterations (nb blocks: block b of the batch's iteration j in lane j * nb + b), and the sweep runs
the pass at a launch's step 0 and on every Q-th step after it.  Every variate keeps the Philox key
of its own (chain, iteration, block, substream), so the draws, the values and the full tune rows
of every chain equal the oracle's -- which knows no batches -- bit for bit, whatever the launch
lengths are against Q: shorter, equal, no multiple (a batch then reaches past the launch's last
iteration and its surplus is dropped), and whatever nb is."""
import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu


def rats(mamba, scheme):
    m = mamba.rats()
    m.setinputs(mamba.model.RATS_DATA)
    return m.setsamplers(scheme)


def run_windows(mamba, m, init, windows, monkeypatch, burnin, thin, seed, chain_offset=0, jit=None):
    """windows: (iterations, MMB_ITERS_PER_LAUNCH or None) each; the engine reads the launch
    length at every run.  Returns the concatenated draws, the values and the tune rows."""
    eng = mamba.Engine(m)
    if jit is not None:
        assert eng.ir_jit()[0] == jit, eng.ir_jit()
    eng.init_chains(init, chain_offset=chain_offset, seed=seed)
    draws = []
    for iters, per_launch in windows:
        if per_launch is None:
            monkeypatch.delenv("MMB_ITERS_PER_LAUNCH", raising=False)
        else:
            monkeypatch.setenv("MMB_ITERS_PER_LAUNCH", str(per_launch))
        d = eng.run(iters, burnin=burnin, thin=thin)
        if d is not None:
            draws.append(d)
    out = np.concatenate(draws), eng.values(), eng.tune()
    eng.close()
    return out


def oracle_run(oracle, m, init, iters, burnin, thin, seed, chain_offset=0):
    st = oracle.new_state(m, init)
    do = oracle.run(m, st, iters, burnin=burnin, thin=thin, seed=seed, chain_offset=chain_offset, nthreads=8)
    return do, st["values"], st["tune"][:, :st["tl"]]


def assert_equal(gpu, ref):
    for x, y in zip(gpu, ref):
        assert x.shape == y.shape
        np.testing.assert_array_equal(x, y)


RAGGED = [(1, 20), (2, 20), (3, 20), (5, 20), (9, 20), (23, 7)]


@pytest.fixture(scope="module")
def ragged_oracle(mamba, oracle):
    m = rats(mamba, mamba.model.rats_scheme_gibbs_amm())
    init = mamba.model.rats_init_ls(20, seed=7)
    return m, init, oracle_run(oracle, m, init, sum(w for w, _ in RAGGED), 3, 2, 19, chain_offset=5000)


@pytest.mark.parametrize("parts", [1, 2])
def test_ragged_launches(mamba, ragged_oracle, monkeypatch, parts):
    """The headline scheme (nb = 7, Q = 4), 20 chains (the last workgroup is half full) with Philox
    chain ids from 5000: single launches of 1, 2, 3, 5 and 9 iterations -- shorter than, equal to
    and no multiple of Q, each starting a batch at an iteration that is no multiple of Q -- then a
    window of 23 iterations as launches of 6, 6, 6 and 5.  thin 2 behind a burnin of 3; as one
    part and as two parts on two streams."""
    m, init, ref = ragged_oracle
    monkeypatch.setenv("MMB_SWEEP_PARTS", str(parts))
    assert_equal(run_windows(mamba, m, init, RAGGED, monkeypatch, 3, 2, 19, chain_offset=5000), ref)


@pytest.mark.parametrize("scheme", ["gibbs_only", "three_blocks"])
def test_other_block_counts(mamba, oracle, monkeypatch, scheme):
    """nb = 5 (bench.scheme_for's gibbs_only: Q = 6, 30 lanes used) and a partial scheme of three
    blocks (s2_c, AMM alpha, mu_alpha: Q = 10, 30 lanes used; the engine accepts a scheme that
    samples only some of the model's nodes, the others keep their initial values).  16 chains,
    windows of 7 and 13 iterations in one launch each: two and three batches at Q = 6, one and two
    at Q = 10, the last one always cut."""
    if scheme == "gibbs_only":
        sch = bench.scheme_for(mamba, "gibbs_only")
    else:
        sch = [mamba.Gibbs("s2_c"), mamba.AMM("alpha", np.eye(30)), mamba.Gibbs("mu_alpha")]
    m = rats(mamba, sch)
    init = mamba.model.rats_init_ls(16, seed=3)
    ref = oracle_run(oracle, m, init, 20, 2, 1, 5)
    assert_equal(run_windows(mamba, m, init, [(7, 20), (13, 20)], monkeypatch, 2, 1, 5), ref)


def test_gamma_replay_inside_a_batch(mamba, oracle, monkeypatch):
    """mmb_gamma_mt replayed in full by single lanes of a batch.  The first Marsaglia-Tsang attempt
    rejects with probability 3.8e-4 at shape 75.001 (s2_c) and 2.0e-3 at shape 15.001 (s2_alpha,
    s2_beta) -- numpy, 2e6 samples each -- so about 4.3e-3 per chain and iteration: 600 chains x
    80 iterations = 48,000 chain-iterations hold about 200 replays, in lanes of every iteration
    of a batch.  A smaller shape would hold none and check nothing: keep K x iterations at this
    size.  Two windows of 45 and 35 iterations at 20 per launch (15 + 15 + 15, 18 + 17), thin 3
    behind a burnin of 6, the fixture of test_gpu_sweep_parts."""
    m = rats(mamba, mamba.model.rats_scheme_gibbs_amm())
    init = mamba.model.rats_init_ls(16384, seed=1000)[:600]
    ref = oracle_run(oracle, m, init, 80, 6, 3, 33)
    assert_equal(run_windows(mamba, m, init, [(45, 20), (35, 20)], monkeypatch, 6, 3, 33), ref)


@pytest.mark.parametrize("kernel", ["specialised", "interpreter"])
def test_node_ir(mamba, oracle, monkeypatch, kernel):
    """The node IR's kernels include the same sweep.h: rats with the headline scheme as traced
    closures (nb = 7, Q = 4), 64 chains, windows of 5 and 6 iterations, through the hipRTC
    specialised kernel -- asserted to be the one that ran -- and through the interpreter."""
    if kernel == "interpreter":
        monkeypatch.setenv("MMB_IR_JIT", "0")
    ir = mamba.ir
    m = ir.rats_model().setinputs(ir.rats_inputs())
    m.setsamplers(ir.rats_scheme_gibbs_amm())
    V = m.init_matrix(ir.rats_inits_ls(64, seed=5), 64)
    ref = oracle_run(oracle, m, V, 11, 2, 1, 11)
    got = run_windows(mamba, m, V, [(5, None), (6, None)], monkeypatch, 2, 1, 11, jit=kernel == "specialised")
    assert_equal(got, ref)
