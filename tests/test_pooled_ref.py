"""tests/pooled_ref.py pinned on the CPU, before tests/test_gpu_pooled.py holds the kernels of
gr.hip and summary.hip to it: hand-computable cases, mpmath for the links, the other restatements
on well-conditioned data (oracle/summary_ref.py, gelman.gelmandiag -- itself pinned to coda's
golden values in tests/test_oracle.py -- and the host shard of tests/test_summary.py), and the
properties the device tests state for their crafted inputs (which link each column selects, which
batch sizes straddle chains, how many ranks a quantile vector reads)."""
import os
import sys

import mpmath
import numpy as np
import pytest

import pooled_ref as pr
from test_summary import HostSummaryShard

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import summary_ref  # noqa: E402

LD = np.longdouble


# ---- hand-computable ---------------------------------------------------------------------
def test_gr_sums_by_hand():
    """Two chains [1, 3] and [2, 6], shift 1: means 2, 4 (phi 1, 3), variances 2, 8."""
    x = np.array([[1.0, 2.0], [3.0, 6.0]]).reshape(2, 1, 2)
    L, sc = pr.gr_sums(x, [0], [1.0])
    np.testing.assert_array_equal(L.astype(float), [2, 4, 10, 10, 68, 2 * 1 + 8 * 3, 2 * 1 + 8 * 9])
    # A = mean |y| + |shift| = 3, 5; |d|^2 sums 2, 8
    np.testing.assert_array_equal(sc.astype(float), [0, 8, 34, 10, 68, 2 * 3 + 8 * 5, 2 * 9 + 8 * 25])


def test_gr_sums_layout_two_columns():
    """p = 2: the p x p blocks are row-major (j, l) and symmetric, the cross terms signed."""
    x = np.empty((2, 2, 2))
    x[:, 0, :] = [[1.0, 2.0], [3.0, 6.0]]
    x[:, 1, :] = [[5.0, 1.0], [1.0, -1.0]]          # means 3, 0; deviations (2, -2), (1, -1)
    L, sc = pr.gr_sums(x, [0, 0], [0.0, 0.0])
    L = L.astype(float)
    assert L[0] == 2 and list(L[1:3]) == [6, 3]
    np.testing.assert_array_equal(L[3:7].reshape(2, 2), [[2 * 2 + 4 * 4, 6], [6, 9]])
    # S2 chain 0: d0 = (-1, 1), d1 = (2, -2): [[2, -4], [-4, 8]]; chain 1: d0 = (-2, 2), d1 = (1, -1): [[8, -4], [-4, 2]]
    np.testing.assert_array_equal(L[7:11].reshape(2, 2), [[10, -8], [-8, 10]])
    np.testing.assert_array_equal(sc.astype(float)[7:11].reshape(2, 2), [[10, 8], [8, 10]])
    np.testing.assert_array_equal(L[11:13], [4 + 64, 64 + 4])            # s2^2
    np.testing.assert_array_equal(L[13:15], [2 * 2 + 8 * 4, 8 * 3 + 0])  # s2 phi
    np.testing.assert_array_equal(L[15:17], [2 * 4 + 8 * 16, 8 * 9 + 0])


def _mp(y):
    """An np.longdouble as an mpmath number, exactly (a double and the rest)."""
    hi = float(y)
    return mpmath.mpf(hi) + mpmath.mpf(float(y - LD(hi)))


def test_links_against_mpmath():
    """The extended-precision links agree with 200-bit mpmath to 2^-61 relative (about 4 of their
    own ulps: the quotient, 1 - x and the log each round once) -- 2^8 below a double's rounding."""
    with mpmath.workprec(200):
        for v in (5e-10, 1.0 - 5e-10, 0.25, 0.75, 1e-300, 0.999):
            want = mpmath.log(mpmath.mpf(v) / (1 - mpmath.mpf(v)))
            assert abs(_mp(pr.link([v], 2)[0]) - want) <= mpmath.mpf(2) ** -61 * abs(want)
        for v in (1e-300, 1e300, 5e-324, np.e, 3.5):
            want = mpmath.log(mpmath.mpf(v))
            assert abs(_mp(pr.link([v], 1)[0]) - want) <= mpmath.mpf(2) ** -61 * abs(want)
    assert pr.link([0.5], 2)[0] == 0 and pr.link([1.0], 1)[0] == 0 and pr.link([-3.0], 0)[0] == -3


def test_link_kinds_by_hand(mamba):
    mm = [[-1.0, 2.0], [0.0, 0.5], [1e-300, 0.5], [0.2, 1.0], [0.2, 0.999], [-0.0, 0.5], [3.0, 4.0]]
    want = [0, 0, 2, 1, 2, 0, 1]
    assert list(pr.link_kinds(mm)) == want and list(mamba.gelman.link_kinds(mm)) == want


def test_chain_partials_by_hand():
    """n = 3, bs = 2: chain 0 holds batch 0 and the first element of batch 1 (tail), chain 1 its
    second element (head) and batch 2; with base 1 the chain at flat 3..5 is head + full."""
    x = np.array([[1.0, 10.0], [2.0, 20.0], [4.0, 40.0]]).reshape(3, 1, 2)
    out, sc = pr.chain_partials(x, [0, 1], 2, [0.0])
    np.testing.assert_array_equal(out[0, 0].astype(float), [7, 21, 1.5, 2.25, 1, 0, 0, 4, 1, 0])
    np.testing.assert_array_equal(out[1, 0].astype(float), [70, 2100, 30, 900, 1, 10, 1, 0, 0, 0])
    np.testing.assert_array_equal(sc[1, 0].astype(float), [70, 2100, 30, 900, 0, 10, 0, 0, 0, 0])
    out, _ = pr.chain_partials(x[:, :, :1], [1], 2, [1.0])               # x' = 0, 1, 3
    np.testing.assert_array_equal(out[0, 0].astype(float), [4, 10, 2, 4, 1, 0, 1, 0, 0, 0])
    out, sc = pr.chain_partials(x[:, :, :1] - 3.0, [1], 7, [0.0])        # inside one batch, not at its start
    np.testing.assert_array_equal(out[0, 0].astype(float), [-2, 6, 0, 0, 0, -2, 3, 0, 0, 0])
    np.testing.assert_array_equal(sc[0, 0].astype(float), [4, 6, 0, 0, 0, 4, 0, 0, 0, 0])
    out, _ = pr.chain_partials(x[:, :, :1], [0], 7, [0.0])               # starts its batch, never closes it: tail
    np.testing.assert_array_equal(out[0, 0].astype(float), [7, 21, 0, 0, 0, 0, 0, 7, 3, 0])


def test_order_stats_and_quantile_by_hand():
    x = np.array([3.0, -1.0, 2.0, 10.0, 0.0]).reshape(5, 1, 1)
    np.testing.assert_array_equal(pr.order_stats(x, 0, [0, 2, 4]), [-1.0, 2.0, 10.0])
    np.testing.assert_array_equal(pr.quantile(x, [0.0, 0.25, 0.5, 0.625, 1.0])[0], [-1.0, 0.0, 2.0, 2.5, 10.0])
    assert pr.quantile_ranks(5, [0.0, 0.625, 1.0]) == [0, 2, 3, 4]
    np.testing.assert_array_equal(pr.minmax(np.array([[-0.0, np.inf], [0.0, -np.inf]]).reshape(2, 2, 1)),
                                  [[0.0, 0.0], [-np.inf, np.inf]])


def test_summarystats_by_hand():
    """Constant within each batch of 2: MCSE = sd(batch values) / sqrt(m); a constant column: 0, 0, NaN."""
    vals = np.array([1.0, 4.0, -2.0, 0.5])
    x = np.stack([np.repeat(vals, 2).reshape(2, 4, order="F"), np.full((2, 4), 2.5)], axis=1)   # vec(x) = chains in turn
    t = pr.summarystats(x, 2)
    v = np.repeat(vals, 2)
    np.testing.assert_allclose(t[0, :4], [v.mean(), v.std(ddof=1), v.std(ddof=1) / np.sqrt(8), vals.std(ddof=1) / 2.0],
                               rtol=1e-15)
    assert t[0, 4] == 2.0                                   # capped at n = 2 iterations
    np.testing.assert_array_equal(t[1, :4], [2.5, 0.0, 0.0, 0.0])
    assert np.isnan(t[1, 4])
    with pytest.raises(ValueError, match="iterations are < 10"):
        pr.summarystats(x, 5)


# ---- against the other restatements, on well-conditioned data --------------------------------
@pytest.mark.parametrize("p", [3, 6])
def test_gr_sums_against_host_gelmandiag(mamba, p):
    """The sums pushed through psrf_from_sums equal the host gelmandiag (pinned to coda) whatever the
    shift; cor_from_sums of the identity sums equals numpy's corrcoef of the pooled draws."""
    x, kinds = pr.gr_end_to_end_inputs(p)
    n = x.shape[0]
    want, wmp = mamba.gelmandiag(x, transform=True, mpsrf=True)
    for shift in (np.zeros(p), pr.mid_shift(x, kinds)):
        L, _ = pr.gr_sums(x, kinds, shift)
        got, mp = mamba.psrf_from_sums(L.astype(np.float64), n, p, mpsrf=True)
        np.testing.assert_allclose(got, want, rtol=1e-9)
        assert mp == pytest.approx(wmp, rel=1e-9)
    ident = np.zeros(p, dtype=np.int32)
    L, _ = pr.gr_sums(x, ident, pr.mid_shift(x, ident))
    pooled = x.transpose(1, 2, 0).reshape(p, -1)
    np.testing.assert_allclose(mamba.cor_from_sums(L.astype(np.float64), n, p), np.corrcoef(pooled), rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("n,K,bs,base", [(60, 9, 7, 0), (60, 9, 100, 3), (17, 5, 17, 0), (17, 5, 18, 7), (16, 3, 1, 2),
                                          (5, 4, 100, 1)])
def test_chain_partials_against_oracle_restatement(n, K, bs, base):
    x = np.random.default_rng(n + K + bs).normal(1.0, 2.0, size=(n, 3, K))
    shift = x.mean(axis=(0, 2))
    kg = base + np.arange(K)
    got, sc = pr.chain_partials(x, kg, bs, shift)
    ref = summary_ref.chain_partials(x, kg, bs, shift)
    np.testing.assert_array_equal(got[:, :, [4, 6, 8, 9]].astype(float), ref[:, :, [4, 6, 8, 9]])
    assert np.all(np.abs(got.astype(float) - ref) <= 1e-13 * sc.astype(float))
    assert np.all(sc[:, :, [4, 6, 8, 9]] == 0)


def test_tables_and_order_statistics_against_oracle_and_host_shard(mamba):
    x = pr.ss_table_inputs(constant=False)
    for bs in pr.SS_TABLE_BS:
        t = pr.summarystats(x, bs)
        # the float64 oracle takes no shift: its batch means at 1e9 carry 1e-7, so column 0 is left
        # to the shifted host path below
        ref = summary_ref.summarystats(x, bs)
        np.testing.assert_allclose(t[1:, :4], ref[1:, :4], rtol=1e-11)
        np.testing.assert_allclose(t[1:, 4], ref[1:, 4], rtol=1e-10)
        host = mamba.summarystats_sharded(HostSummaryShard(x), batch_size=bs)
        np.testing.assert_allclose(host[:, :4], t[:, :4], rtol=1e-10)
        np.testing.assert_allclose(host[:, 4], t[:, 4], rtol=1e-8)
    xo = pr.os_inputs(infinite=False)
    for q in (pr.Q12, pr.Q_ENDS):
        np.testing.assert_array_equal(pr.quantile(xo, q), summary_ref.quantile(xo, q))
        np.testing.assert_array_equal(pr.quantile(xo, q), mamba.quantile_sharded(HostSummaryShard(xo), q))
    xi = pr.os_inputs(infinite=True)
    N = xi.shape[0] * xi.shape[2]
    for j in range(4):
        np.testing.assert_array_equal(mamba.summary.order_stats(HostSummaryShard(xi), j, range(N)),
                                      pr.order_stats(xi, j, range(N)))
    np.testing.assert_array_equal(HostSummaryShard(xi).gr_range(), pr.minmax(xi))


# ---- the stated properties of the device tests' inputs -----------------------------------------
def test_gr_inputs_are_as_stated():
    assert sorted(set(pr.GR_SHAPES)) == sorted([(1, 2), (1, 255), (1, 257), (2, 2), (2, 255), (2, 257), (4, 2), (4, 255),
                                                (4, 257), (5, 15), (5, 17), (64, 33)])
    assert pr.GR_LENGTHS == (2, 31, 33, 65) and len(pr.all_gr_cases()) == 48
    for p, K in pr.GR_SHAPES:
        assert p <= pr.GR_SMALL_MAX or (pr.GR_SMALL_MAX < p <= pr.GR_BIG_MAX)
        seen, levels = set(), set()
        for n in pr.GR_LENGTHS:
            assert n + K < 2 ** 15
            x, kinds = pr.gr_inputs(p, K, n)
            assert x.shape == (n, p, K) and np.all(np.isfinite(x))
            assert len(set(kinds)) == min(p, 3)                       # a mix wherever there is room for one
            seen |= {(j, int(kinds[j])) for j in range(p)}
            assert np.all(x[:, :, pr.CONSTANT_CHAIN] == x[0, :, pr.CONSTANT_CHAIN])
            y = np.stack([pr.link(x[:, j, :], int(kinds[j])) for j in range(p)], axis=1)
            assert np.all(np.isfinite(y.astype(float)))
            d = np.abs(y - y.mean(0)[None])
            for j in range(p):
                c = x[:, j, :]
                if kinds[j] == 2:
                    assert 0.0 < c.min() <= 1e-9 and 1.0 - 1e-9 <= c.max() < 1.0
                elif kinds[j] == 1:
                    assert c.min() == 1e-300 and c.max() == 1e300
                else:
                    lv = pr.gr_level(j, n)
                    levels.add(lv)
                    assert np.all(np.abs(c - lv) < 8.0) and np.ptp(c[:, 0]) > 1e-3        # unit spread about the level
                # the condition of the S2 scale: a link's rounding of y (relative to |y|) stays
                # relative to the deviations too, in every chain but the constant one
                if kinds[j] != 0:
                    live = np.delete(np.arange(K), pr.CONSTANT_CHAIN)
                    assert np.all(np.abs(y[:, j, live]).max(0) <= 1e4 * d[:, j, live].mean(0))
        # over the lengths column 0 goes through every link kind, and some identity column sits at 1e8
        assert {k for j, k in seen if j == 0} == {0, 1, 2}
        # (a single column is identity at one length only; from p = 4 on both levels occur)
        assert 1e8 in levels and (p < 4 or levels == {0.0, 1e8})
    # the big kernel's edges: chain counts on both sides of a multiple of 16, and one workgroup's last chunk partial
    assert {K % pr.GR_BIG_CHAINS for p, K in pr.GR_SHAPES if p > pr.GR_SMALL_MAX} == {15, 1}
    assert {n % pr.GR_TI for n in pr.GR_LENGTHS} == {2, 31, 1}


@pytest.mark.parametrize("p", [3, 6])
def test_gr_end_to_end_inputs_select_the_stated_links(mamba, p):
    x, kinds = pr.gr_end_to_end_inputs(p)
    mm = pr.minmax(x)
    assert list(pr.link_kinds(mm)) == list(kinds) == list(mamba.gelman.link_kinds(mm))
    assert set(kinds) == {0, 1, 2}
    if p == 6:
        assert mm[3, 0] == 0.0 and kinds[3] == 0 and not np.signbit(mm[3, 0])
        assert mm[4, 1] == 1.0 and mm[4, 0] > 0.0 and kinds[4] == 1
        assert mm[5, 1] < 0.0


def test_chain_summary_inputs_are_as_stated():
    assert sorted(pr.SS_SHAPES) == sorted((p, K) for p in (1, 3, 64) for K in (1, 255, 257))
    assert pr.SS_LENGTHS == (1, 15, 16, 17, 100) and pr.SS_BASES == (0, 7)
    assert {n % pr.SS_U for n in pr.SS_LENGTHS} >= {1, 15, 0, 4} and {K - pr.SS_THREADS for K in (255, 257)} == {-1, 1}
    for p, K in pr.SS_SHAPES:
        cols = set()
        for n in pr.SS_LENGTHS:
            bss = pr.ss_batch_sizes(n, K)
            assert {1, n, n + 1} <= set(bss) and max(bss) > n + 1
            primes = [b for b in bss if b in (3, 5, 7, 11, 13, 17, 19) and n % b and (n * K) % b]
            assert primes
            assert any((7 * n) % b for b in bss)                      # base 7: the shard starts inside a batch
            x = pr.ss_inputs(p, K, n)
            for j in range(p):
                kind = pr.ss_column(j, n)
                cols.add(kind)
                c = x[:, j, :]
                if kind == "level 1e9":
                    assert abs(c.mean() - 1e9) < 1e-2 and (c.size == 1 or c.std() < 1e-2)
                elif kind == "constant":
                    assert np.all(c == 2.5)
                else:
                    assert np.all(c * 2 == np.round(c * 2)) and (c.size < 30 or (np.unique(c).size < 20 and c.min() < 0 < c.max()))
        assert cols == set(pr.SS_COLUMNS)                             # also at p = 1, over the lengths
    for const in (False, True):
        x = pr.ss_table_inputs(const)
        n, p, K = x.shape
        assert p == 3 + const
        for bs in pr.SS_TABLE_BS:
            assert (n * K) // bs >= 2
        assert (n * K) // pr.SS_TABLE_BS_TOO_BIG < 2
    flat = pr.SS_TABLE_SPLIT * 60
    assert [flat % bs != 0 for bs in pr.SS_TABLE_BS] == [True, False, True]


def test_wide_model_monitors_66_values(mamba):
    """The node-IR model of the device tests lowers to 66 monitored columns (no engine is made)."""
    from test_gpu_pooled import wide_model
    m = wide_model(mamba)
    K = 5
    assert m.init_matrix(mamba.ir.rats_inits_ls(K, seed=2), K).shape[0] == K
    assert m.ir().nmon == 8 and len(m.monitor_names) == 66 == pr.wide_inputs().shape[1]
    assert m.monitor_names[0] == "alpha[1]" and m.monitor_names[30] == "alpha0" and m.monitor_names[-1] == "s2_c"


def test_order_statistic_inputs_are_as_stated():
    for inf in (False, True):
        x = pr.os_inputs(inf)
        assert x[:, 0].min() < 0 < x[:, 0].max() and np.unique(x[:, 1]).size == 1 and np.unique(x[:, 2]).size == 3
        c = x[:, 3].ravel()
        z = c[c == 0.0]
        assert np.signbit(z).any() and not np.signbit(z).all()
        for v in (pr.TINY, -pr.TINY, 1.7e308, -1.7e308):
            assert (c == v).any()
        assert np.isinf(c).any() == inf and not np.isnan(x).any()
    assert pr.TINY > 0 and pr.TINY / 2 == 0
    for N in (37 * 11, 2 * pr.OS_BIG_K, 9 * 5):
        assert len(pr.Q12) == 12 and len(pr.quantile_ranks(N, pr.Q12)) > 16
    assert pr.quantile_ranks(407, pr.Q_ENDS) == [0, 203, 406]
    xb = pr.os_big_inputs(2)
    assert xb.shape == (2, 1, 16384 + 257) and xb[:, :, 16384:].min() > xb[:, :, :16384].max()
    xw = pr.os_wide_inputs()
    assert xw.shape[1] == 64 and abs(xw[:, 63].mean() - 63) < 1
    assert pr.wide_inputs().shape == (40, 66, 5) and 200 // 10 >= 2
    for p, n, K in ((1, 1, 1), (64, 3, 5), (66, 3, 5), (1, 8, pr.OS_BIG_K)):
        x = pr.range_inputs(p, n, K)
        mm = pr.minmax(x)
        assert mm[0, 1] == np.inf and (n * K == 1 or mm[0, 0] == -np.inf)
        if p > 2:
            assert np.all(x[:, 1] == 0) and np.signbit(x[:, 1]).any() and not np.signbit(x[:, 1]).all() and mm[2, 1] == 0
    assert 8 * pr.OS_BIG_K > 512 * 256 > 3 * 5                        # the range kernel's stride loop iterates / does not
