"""The pooled post-processing kernels on the device, on draws the test writes itself
(Engine.set_draws; no sampler runs): gr.hip (gr_stats_kernel<1..4>, gr_stats_big_kernel,
gr_range_kernel) and summary.hip (ss_chain_kernel, os_hist_kernel) against the extended-precision
restatement tests/pooled_ref.py, which tests/test_pooled_ref.py pins on the CPU together with the
stated properties of every crafted input used here.

Tolerances.  Sums: |got - ref| <= 1e-10 x scale per entry, scale being the sum of the absolute
values of the terms added (pooled_ref's docstrings say which terms); 1e-10 is the factor of
tests/test_gpu_diag.py check_autocov and of the summary tests' rtol, about 2^20 roundings, where
the longest sum here (n + K < 2^15 terms) can lose 2^15.  Counts, ranges, order statistics and
quantiles are compared exactly.  Every sums test prints the largest error / bound it saw.

A logistic engine with a handful of observations gives any width 1 <= p <= 64; wider needs a
node-IR model (rats with every node monitored: 66 columns), built with the interpreter kernel so
that nothing is compiled at creation."""
import threading

import numpy as np
import pytest

import pooled_ref as pr

pytestmark = pytest.mark.gpu
LD = np.longdouble


# ---- harness -----------------------------------------------------------------------------
def logistic_engine(mamba, p, K):
    nobs = 4
    m = mamba.logistic(nobs, p, 10.0)
    m.setinputs({"X": np.random.default_rng(p).normal(size=(nobs, p)), "y": np.array([0.0, 1.0, 1.0, 0.0])})
    m.setsamplers([mamba.NUTS("beta", dtype="analytic")])
    eng = mamba.Engine(m)
    eng.init_chains(np.zeros((K, p)), seed=1)
    assert eng.pmon == p
    return m, eng


def wide_model(mamba):
    """doc/examples/rats.jl through the node IR with every node but y monitored: alpha (30), alpha0,
    mu_alpha, s2_alpha, beta (30), mu_beta, s2_beta, s2_c = 66 columns."""
    ir = mamba.ir
    m = ir.Model(
        y=ir.Stochastic(1, lambda alpha, beta, rat, Xm, s2_c: ir.MvNormal(alpha[rat] + beta[rat] * Xm, ir.sqrt(s2_c)),
                        False),
        alpha=ir.Stochastic(1, lambda mu_alpha, s2_alpha: ir.Normal(mu_alpha, ir.sqrt(s2_alpha))),
        alpha0=ir.Logical(lambda mu_alpha, xbar, mu_beta: mu_alpha - xbar * mu_beta),
        mu_alpha=ir.Stochastic(lambda: ir.Normal(0.0, 1000)),
        s2_alpha=ir.Stochastic(lambda: ir.InverseGamma(0.001, 0.001)),
        beta=ir.Stochastic(1, lambda mu_beta, s2_beta: ir.Normal(mu_beta, ir.sqrt(s2_beta))),
        mu_beta=ir.Stochastic(lambda: ir.Normal(0.0, 1000)),
        s2_beta=ir.Stochastic(lambda: ir.InverseGamma(0.001, 0.001)),
        s2_c=ir.Stochastic(lambda: ir.InverseGamma(0.001, 0.001)))
    return m.setinputs(ir.rats_inputs()).setsamplers(mamba.model.rats_scheme_reference())


@pytest.fixture(scope="module")
def engines(mamba):
    """(p, K) -> (model, engine), made once; a test uploads the draws it needs."""
    made = {}

    def get(p, K):
        if (p, K) not in made:
            made[p, K] = logistic_engine(mamba, p, K)
        return made[p, K]

    yield get
    for _, eng in made.values():
        eng.close()


def chains_of(mamba, m, eng, x):
    eng.set_draws(x)
    return mamba.Chains(x, m.monitor_names, 1, 1, np.arange(1, x.shape[2] + 1), m, eng)


def check_scaled(got, ref, scale, exact, what):
    """|got - ref| <= 1e-10 scale entry by entry, the entries `exact` (a mask) equal; returns
    the largest error / bound over the entries with a bound."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape and np.all(np.isfinite(got)), what
    np.testing.assert_array_equal(got[exact], ref[exact].astype(np.float64), err_msg=what)
    err = np.abs(got.astype(LD) - ref)
    bound = LD(1e-10) * scale
    bad = (err > bound) & ~exact
    live = (bound > 0) & ~exact
    ratio = float((err[live] / bound[live]).max()) if live.any() else 0.0
    assert not bad.any(), (f"{what}: {int(bad.sum())} entries beyond 1e-10 x scale, first at {np.argwhere(bad)[0]}: "
                           f"got {got[bad][0]!r}, ref {ref[bad][0]!r}, scale {scale[bad][0]!r}; largest ratio {ratio:.3g}")
    return ratio


# ---- Gelman-Rubin sums -----------------------------------------------------------------------
@pytest.mark.parametrize("p,K", pr.GR_SHAPES)
def test_gr_partials(engines, p, K):
    """gr_stats_kernel<p> for p = 1, 2, 4 over chain counts inside and across a 256-thread block,
    gr_stats_big_kernel at its narrowest (5) and widest (64: all 4096 thread-owned pairs) with chain
    counts that are no multiple of its 16-chain chunk; lengths 2 (the shortest a covariance has)
    and on both sides of the 32-iteration LDS tile; mixed link kinds with values at the edges of
    their domains, a constant chain, a column at 1e8; under a zero shift and the mid-range one."""
    _, eng = engines(p, K)
    worst = 0.0
    exact = None
    for n in pr.GR_LENGTHS:
        x, kinds = pr.gr_inputs(p, K, n)
        eng.set_draws(x)
        for shift in (np.zeros(p), pr.mid_shift(x, kinds)):
            ref, scale = pr.gr_sums(x, kinds, shift)
            if exact is None:
                exact = np.zeros(ref.size, dtype=bool)
                exact[0] = True
            got = eng.gr_partials(kinds, shift)
            worst = max(worst, check_scaled(got, ref, scale, exact, f"p={p} K={K} n={n} kinds={list(kinds)}"))
    print(f"gr_partials p={p} K={K}: largest error / bound = {worst:.3g}")


@pytest.mark.parametrize("p", [3, 6])
def test_gelmandiag_and_cor_end_to_end(mamba, engines, p):
    """gelmandiag(transform=True, mpsrf=True) and cor from the device sums against the reference's
    sums through the same closing formulas; the draws make link() choose all three kinds, with a
    minimum of exactly 0.0 (identity, not log) and a maximum of exactly 1.0 (log, not logit)."""
    x, kinds = pr.gr_end_to_end_inputs(p)
    n = x.shape[0]
    _, eng = engines(p, x.shape[2])
    eng.set_draws(x)
    np.testing.assert_array_equal(eng.gr_range(), pr.minmax(x))
    ps, mp = mamba.gelmandiag_sharded(eng, transform=True, mpsrf=True)
    L, _ = pr.gr_sums(x, kinds, pr.mid_shift(x, kinds))
    want, wmp = mamba.psrf_from_sums(L.astype(np.float64), n, p, mpsrf=True)
    np.testing.assert_allclose(ps, want, rtol=1e-8)
    np.testing.assert_allclose(mp, wmp, rtol=1e-8)
    ident = np.zeros(p, dtype=np.int32)
    L, _ = pr.gr_sums(x, ident, pr.mid_shift(x, ident))
    np.testing.assert_allclose(mamba.cor_sharded(eng), mamba.cor_from_sums(L.astype(np.float64), n, p), rtol=1e-8)
    ps0, _ = mamba.gelmandiag_sharded(eng, transform=False)           # and untransformed: identity everywhere
    L, _ = pr.gr_sums(x, ident, pr.mid_shift(x, ident))
    np.testing.assert_allclose(ps0, mamba.psrf_from_sums(L.astype(np.float64), n, p)[0], rtol=1e-8)


# ---- range ---------------------------------------------------------------------------------
@pytest.mark.parametrize("p,n,K", [(1, 1, 1), (64, 3, 5), (1, 8, pr.OS_BIG_K)])
def test_gr_range(engines, p, n, K):
    """Exact minima and maxima with -0.0 / +0.0 and +-inf among the draws: fewer elements than the
    launch has threads, and more (8 x 16641 > 512 x 256: the stride loop iterates)."""
    x = pr.range_inputs(p, n, K)
    _, eng = engines(p, K)
    eng.set_draws(x)
    np.testing.assert_array_equal(eng.gr_range(), pr.minmax(x))


# ---- chain summaries -------------------------------------------------------------------------
SS_EXACT = np.array([f in ("nfull", "hcnt", "tcnt", "pad") for f in pr.FIELDS])


@pytest.mark.parametrize("p,K", pr.SS_SHAPES)
def test_chain_summary(engines, p, K):
    """ss_chain_kernel field by field: lengths around its 16-deep unroll and n = 1, chain counts
    inside and across a 256-thread block, batch sizes 1, n, n + 1, a prime that straddles every
    chain and one longer than a chain, shards that start at chain 0 and at chain 7 (inside a batch),
    shift 0 and the column mean; a column at 1e9, a constant one and one of heavy ties."""
    _, eng = engines(p, K)
    worst = 0.0
    for n in pr.SS_LENGTHS:
        x = pr.ss_inputs(p, K, n)
        eng.set_draws(x)
        for shift in (np.zeros(p), x.mean(axis=(0, 2))):
            for bs in pr.ss_batch_sizes(n, K):
                for base in pr.SS_BASES:
                    ref, scale = pr.chain_partials(x, base + np.arange(K), bs, shift)
                    got = eng.chain_summary(shift, bs, base)
                    exact = np.broadcast_to(SS_EXACT, ref.shape)
                    worst = max(worst, check_scaled(got, ref, scale, exact, f"p={p} K={K} n={n} bs={bs} base={base}"))
    print(f"chain_summary p={p} K={K}: largest error / bound = {worst:.3g}")


def check_table(got, ref):
    """The tolerances of tests/test_gpu_parity.py test_device_summarystats_and_quantiles."""
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    np.testing.assert_allclose(got[:, :4], ref[:, :4], rtol=1e-10)
    np.testing.assert_allclose(got[:, 4], ref[:, 4], rtol=1e-8)


class InProcess:
    """The two collectives of pool_summary among `world` threads of one process."""

    def __init__(self, world):
        self.slots = [None] * world
        self.bar = threading.Barrier(world, timeout=60)

    def gather(self, rank, obj):
        self.slots[rank] = obj
        self.bar.wait()
        out = list(self.slots)
        self.bar.wait()
        return out

    def allreduce_sum(self, rank, x):
        g = self.gather(rank, np.asarray(x, dtype=np.float64))
        return sum(g[1:], g[0] * 1.0)                     # in rank order: the same bits on every rank


@pytest.mark.parametrize("bs", pr.SS_TABLE_BS)
def test_summary_pooled_over_two_shards(mamba, engines, bs):
    """One draw array over two engines, split at a chain boundary inside a batch (bs 7 and 100; 60
    puts it on a batch edge): the partials of both, pooled by summary.pool_summary with in-process
    collectives, give the table of the whole array on both ranks."""
    x = pr.ss_table_inputs(constant=False)
    n, p, K = x.shape
    cut = pr.SS_TABLE_SPLIT
    shift = x.mean(axis=(0, 2))
    parts = []
    for lo, hi in ((0, cut), (cut, K)):
        _, eng = engines(p, hi - lo)
        eng.set_draws(x[:, :, lo:hi])
        parts.append((eng.chain_summary(shift, bs, lo), lo + np.arange(hi - lo)))
    coll = InProcess(2)
    out, errs = [None, None], []

    def rank(r):
        try:
            out[r] = mamba.pool_summary(parts[r][0], parts[r][1], n, bs, shift,
                                        allreduce_sum=lambda v: coll.allreduce_sum(r, v),
                                        allgather=lambda v: coll.gather(r, v))
        except Exception as e:   # a broken barrier on the other rank follows from the first error
            errs.append(e)
            coll.bar.abort()

    th = [threading.Thread(target=rank, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    ref = pr.summarystats(x, bs)
    check_table(out[0], ref)
    np.testing.assert_array_equal(out[0], out[1])


def test_summarystats_single_engine(mamba, engines):
    """Chains.summarystats against the reference table; the constant column gives SD = MCSE = 0
    and ESS NaN exactly where the reference does; too few batches are an ArgumentError."""
    x = pr.ss_table_inputs(constant=True)
    m, eng = engines(x.shape[1], x.shape[2])
    sim = chains_of(mamba, m, eng, x)
    for bs in pr.SS_TABLE_BS:
        got, ref = sim.summarystats(bs), pr.summarystats(x, bs)
        check_table(got, ref)
        np.testing.assert_array_equal(got[1], [2.5, 0.0, 0.0, 0.0, np.nan])
    with pytest.raises(mamba.ArgumentError, match="iterations are <"):
        sim.summarystats(pr.SS_TABLE_BS_TOO_BIG)


# ---- order statistics and quantiles ------------------------------------------------------------
def test_order_stats_every_rank(mamba, engines):
    """Every rank of every column at once (407 targets: 26 launches of at most 16 per pass): mixed
    signs, an all-equal column, three distinct values, and signed zeros, the smallest subnormals,
    +-1.7e308 and +-inf in one column."""
    x = pr.os_inputs(infinite=True)
    _, eng = engines(x.shape[1], x.shape[2])
    eng.set_draws(x)
    N = x.shape[0] * x.shape[2]
    for j in range(x.shape[1]):
        np.testing.assert_array_equal(mamba.summary.order_stats(eng, j, range(N)), pr.order_stats(x, j, range(N)))
        np.testing.assert_array_equal(mamba.summary.order_stats(eng, j, [N - 1, 0, 0]), pr.order_stats(x, j, [N - 1, 0, 0]))
    for r in (N, N + 5):
        with pytest.raises(mamba.ArgumentError, match="out of range"):
            mamba.summary.order_stats(eng, 0, [0, r])


def test_quantiles(mamba, engines):
    """q = 0 and 1, and 12 probabilities that read 24 distinct ranks (two launches per pass)."""
    x = pr.os_inputs(infinite=False)
    m, eng = engines(x.shape[1], x.shape[2])
    sim = chains_of(mamba, m, eng, x)
    for q in (pr.Q_ENDS, pr.Q12, pr.Q12 + pr.Q_ENDS):
        np.testing.assert_array_equal(sim.quantile(q), pr.quantile(x, q))


def test_one_draw(mamba, engines):
    x = np.full((1, 1, 1), -0.0)
    m, eng = engines(1, 1)
    sim = chains_of(mamba, m, eng, x)
    np.testing.assert_array_equal(mamba.summary.order_stats(eng, 0, [0]), [0.0])
    np.testing.assert_array_equal(sim.quantile(pr.Q12 + pr.Q_ENDS), pr.quantile(x, pr.Q12 + pr.Q_ENDS))
    with pytest.raises(mamba.ArgumentError, match="out of range"):
        mamba.summary.order_stats(eng, 0, [1])
    np.testing.assert_array_equal(eng.gr_range(), [[0.0, 0.0]])


def test_order_stats_more_chains_than_one_grid_stride(mamba, engines):
    """16384 + 257 chains: os_hist_kernel's grid is capped at 64 x 256 chains, the rest is reached by
    its stride loop -- and holds all the largest values."""
    x = pr.os_big_inputs(2)
    m, eng = engines(1, pr.OS_BIG_K)
    sim = chains_of(mamba, m, eng, x)
    N = 2 * pr.OS_BIG_K
    ranks = [0, 1, N // 2, N - 2 * 257 - 1, N - 2 * 257, N - 2, N - 1] + pr.quantile_ranks(N, pr.Q12)
    np.testing.assert_array_equal(mamba.summary.order_stats(eng, 0, ranks), pr.order_stats(x, 0, ranks))
    np.testing.assert_array_equal(sim.quantile(pr.Q12 + pr.Q_ENDS), pr.quantile(x, pr.Q12 + pr.Q_ENDS))
    with pytest.raises(mamba.ArgumentError, match="out of range"):
        mamba.summary.order_stats(eng, 0, [N])


def test_order_stats_wide(mamba, engines):
    """64 columns: a nonzero column index, the last one included, selects that column alone."""
    x = pr.os_wide_inputs()
    m, eng = engines(64, x.shape[2])
    sim = chains_of(mamba, m, eng, x)
    N = x.shape[0] * x.shape[2]
    for j in (1, 31, 63):
        np.testing.assert_array_equal(mamba.summary.order_stats(eng, j, range(N)), pr.order_stats(x, j, range(N)))
    np.testing.assert_array_equal(sim.quantile(pr.Q12), pr.quantile(x, pr.Q12))


# ---- more than 64 monitored values ---------------------------------------------------------------
def test_66_monitored_values(mamba, monkeypatch):
    """A node-IR model that monitors 66 values: the range, summarystats and quantile serve it (the
    range reduction once kept its result in a 64-column host array); the Gelman-Rubin sums refuse it
    by name, through every caller, and leave the engine usable."""
    monkeypatch.setenv("MMB_IR_JIT", "0")
    m = wide_model(mamba)
    x = pr.wide_inputs()
    K = x.shape[2]
    V = m.init_matrix(mamba.ir.rats_inits_ls(K, seed=2), K)          # compiles the node IR
    eng = mamba.Engine(m)
    assert eng.pmon == 66 and not eng.ir_jit()[0]
    eng.init_chains(V, seed=3)
    sim = chains_of(mamba, m, eng, x)
    np.testing.assert_array_equal(eng.gr_range(), pr.minmax(x))
    big = pr.range_inputs(66, 3, K)
    eng.set_draws(big)
    np.testing.assert_array_equal(eng.gr_range(), pr.minmax(big))
    eng.set_draws(x)
    first = sim.summarystats(10)
    check_table(first, pr.summarystats(x, 10))
    np.testing.assert_array_equal(sim.quantile(pr.Q12 + pr.Q_ENDS), pr.quantile(x, pr.Q12 + pr.Q_ENDS))
    refusal = "at most 64 monitored values; this model monitors 66"
    for call in (lambda: mamba.gelmandiag_sharded(eng, transform=True, mpsrf=True), lambda: sim.cor(),
                 lambda: eng.gr_partials(np.zeros(66, dtype=np.int32), np.zeros(66))):
        with pytest.raises(RuntimeError, match=refusal):
            call()
    comm = mamba.Comm([eng])
    try:
        np.testing.assert_array_equal(comm.range_allreduce(), pr.minmax(x))
        with pytest.raises(RuntimeError, match=refusal):
            mamba.gelmandiag_rccl(comm, transform=True)
    finally:
        comm.close()
    np.testing.assert_array_equal(sim.summarystats(10), first)
    np.testing.assert_array_equal(eng.gr_range(), pr.minmax(x))
    eng.close()
