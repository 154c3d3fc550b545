"""heideldiag, rafterydiag and cor without a GPU: the C ABI's null-engine rejection, the Python
argument errors, the restatement tests/heidel_raftery_ref.py pinned by known values and closed
forms, and the host formulas of mamba.jl_amd/diag.py / gelman.py fed by an engine-shaped host
shard (heidel_raftery_ref.HostShard).  The kernels are checked in tests/test_gpu_heidel_raftery.py."""
import ctypes as C
import math
import warnings

import numpy as np
import pytest

import heidel_raftery_ref as hr

Q, R, S = 0.1, 0.05, 0.9            # Nmin 98: the Raftery-Lewis loop runs on a few hundred draws


def test_entry_points_reject_null(mamba):
    lib = mamba.abi.lib()
    out = np.zeros(64)
    starts = (C.c_int64 * 2)(0, 4)
    for rc in (lib.mmb_chain_cvm(None, 2, starts, mamba.abi.dptr(out)),
               lib.mmb_chain_mcse_from(None, starts, 8, mamba.abi.MMB_MCSE_IMSE, 100, mamba.abi.dptr(out)),
               lib.mmb_chain_raftery(None, 0.1, mamba.abi.dptr(out))):
        assert rc == -1
        assert b"null" in lib.mmb_last_error(None)
    assert (mamba.abi.MMB_HEIDEL_MAX_STARTS, mamba.abi.MMB_RAFTERY_FIELDS, mamba.abi.MMB_ABI_VERSION) == (16, 8, 10)


def test_pcramer_known_values(mamba):
    """The 95 % and 99 % points of the Cramer-von Mises distribution (0.46136, 0.74346), to the
    accuracy of the four-term series."""
    for f in (hr.pcramer, mamba.pcramer):
        assert float(f(0.46136)) == pytest.approx(0.95, abs=1e-4)
        assert float(f(0.74346)) == pytest.approx(0.99, abs=1e-4)
    x = np.array([[0.05, 0.3], [1.0, 2.5]])
    np.testing.assert_allclose(mamba.pcramer(x), np.vectorize(hr.pcramer)(x), rtol=1e-14)
    assert math.isnan(hr.pcramer(float("nan"))) and np.isnan(mamba.pcramer(np.array([np.nan]))).all()


@pytest.mark.parametrize("n,count", [(10, 4), (19, 9), (20, 5), (400, 5)])
def test_candidate_windows(mamba, n, count):
    """i = 1, 1 + trunc(0.1 n), ... while i < n / 2 (heideldiag.jl:6-10): 0-based multiples of delta."""
    starts, i_final = mamba.diag.heidel_starts(n)
    assert (starts, i_final) == hr.heidel_starts(n)
    delta = int(0.10 * n)
    assert len(starts) == count <= 9 and starts == [j * delta for j in range(count)]
    assert i_final >= n / 2 and i_final - delta < n / 2


def test_ref_heidel_constant_series():
    """S0 = 0 and W = 0: I = 0/0, the p-value is NaN, no window converges; halfwidth 0 and
    0 / 1.5 <= eps.  n = 40: i = 1, 5, ..., 17, then 21."""
    vals, side = hr.heideldiag(np.full(40, 1.5), start=1)
    assert vals[0] == 20.0 and vals[1] == 0.0 and math.isnan(vals[2]) and vals[3:] == [1.5, 0.0, 1.0]
    assert hr.cvm(np.full(7, -3.25)) == (-3.25, 0.0)
    assert side["pgap"] == math.inf


def test_ref_heidel_linear_ramp():
    """A ramp of 400 never converges (its last window's p-value is 0.0425): Burn-in is the first
    i >= n / 2, 201, + start - 2, and the p-value, mean and halfwidth are the last tested window's,
    x[161:400] (the mean of 160 .. 399)."""
    x = np.arange(400.0)
    for start in (1, 5):
        vals, side = hr.heideldiag(x, start=start)
        assert vals[0] == 201 + start - 2 and vals[1] == 0.0 and vals[2] == 0.0425
        assert vals[3] == 279.5 and side["start"] == 160 and vals[5] == 0.0
        assert vals[4] == pytest.approx(math.sqrt(2.0) * 1.3859038243496777 * hr.diag_ref.mcse(x[160:], "imse")["mcse"],
                                        rel=1e-12)
    # B_t of a ramp of length m: -t (m - t) / 2, so W = sum t^2 (m - t)^2 / (4 m^2)
    m = 240
    t = np.arange(1, m + 1, dtype=float)
    assert hr.cvm(x[160:])[1] == pytest.approx(np.sum(t * t * (m - t) ** 2) / (4.0 * m * m), rel=1e-13)


def test_ref_raftery_constant_series():
    """dichot is all ones: the one populated cell fits exactly, g2 = 0, bic = -2 log(n - 2) < 0 at
    kthin = 1; alpha = 0/0, so Burn-in and Total are NaN."""
    f, least = hr.raftery_counts(np.full(200, 1.5), Q)
    assert f[:7] == [1.5, 1.0, 200.0, 0.0, 0.0, 0.0, 199.0]
    assert f[7] == pytest.approx(-2.0 * math.log(198.0), rel=1e-15) and least == abs(f[7])
    vals, _ = hr.rafterydiag(np.full(200, 1.5), Q, R, S)
    assert vals[0] == 1.0 and math.isnan(vals[1]) and math.isnan(vals[2]) and vals[3] == 98.0 and math.isnan(vals[4])


def test_ref_raftery_alternating_dichotomy():
    """x_t = (-1)^t, n = 200, q = 0.1: the threshold is -1 and dichot = 0, 1, 0, 1, ...: the two
    populated triples fit exactly (bic < 0 at kthin = 1), n01 = 100, n10 = 99, alpha = beta = 1,
    so m = log(2 eps) / log(|1 - 2|) = -6.2 / 0 = -Inf as Julia's float division gives it, and
    n = 0: Burn-in, Total and the dependence factor are -Inf."""
    x = np.array([(-1.0) ** t for t in range(200)])
    f, _ = hr.raftery_counts(x, Q)
    assert f[:7] == [-1.0, 1.0, 200.0, 0.0, 99.0, 100.0, 0.0]
    vals, _ = hr.rafterydiag(x, Q, R, S, start=11, thin=2)
    assert vals == [2.0, -math.inf, -math.inf, 98.0, -math.inf]
    # and a series that runs out of elements before bic turns negative: kthin NaN, zero counts
    # (dichot 1, 1, 0, 0, 1: g2 = 4 log 2 > 2 log 3 at kthin = 1; 1, 0, 1 gives bic = 0 at kthin = 2;
    # two elements are left at kthin = 3)
    f, least = hr.raftery_counts(np.array([0.0, 0.0, 5.0, 5.0, 0.0]), 0.5)
    assert f[0] == 0.0 and math.isnan(f[1]) and f[2:7] == [2.0, 0.0, 0.0, 0.0, 0.0] and math.isnan(f[7])
    assert least == 0.0


def test_ref_quantile_is_julias():
    x = np.array([4.0, 1.0, 3.0, 2.0, 5.0])
    assert hr.quantile(x, 0.5) == 3.0 and hr.quantile(x, 0.1) == 1.4 and hr.quantile(x, 0.25) == 2.0
    np.testing.assert_allclose([hr.quantile(x, q) for q in (0.3, 0.77)], np.quantile(x, (0.3, 0.77)), rtol=1e-15)


def _shard():
    """Eight chains of input B: four with the transient, and the two of which one series fails."""
    return hr.HostShard(hr.input_b()[:, :, [4, 5, 6, 7, 20, 21, 25, 26]])


@pytest.mark.parametrize("etype", ["imse", "ipse", "bm"])
def test_heideldiag_host_formula(mamba, etype):
    sh = _shard()
    got = mamba.heideldiag(sh, etype=etype, batch_size=5, start=3)
    ref, _ = hr.heideldiag_chains(sh.d, etype=etype, size=5, start=3)
    assert got.shape == (3, 6, 8)
    np.testing.assert_array_equal(got[:, [0, 1, 5], :], ref[:, [0, 1, 5], :])
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0, equal_nan=True)
    assert len(np.unique(got[:, 0, :])) > 2 and (got[:, 1, :] == 0).any()     # several windows, a failure


def test_heideldiag_constant_and_ramp(mamba):
    d = np.empty((400, 2, 1))
    d[:, 0, 0] = 1.5
    d[:, 1, 0] = np.arange(400.0)
    got = mamba.heideldiag(hr.HostShard(d), start=7)
    ref, _ = hr.heideldiag_chains(d, start=7)
    np.testing.assert_array_equal(got, ref)
    assert got[0, 0, 0] == got[1, 0, 0] == 201 + 7 - 2
    np.testing.assert_array_equal(got[0, 1:, 0], [0.0, np.nan, 1.5, 0.0, 1.0])


def test_rafterydiag_host_formula(mamba):
    v = hr.input_c()[:, :, :6]
    sh = hr.HostShard(v)
    got = mamba.rafterydiag(sh, Q, R, S, start=101, thin=2)
    ref, _ = hr.rafterydiag_chains(v, Q, R, S, start=101, thin=2)
    assert got.shape == (3, 5, 6)
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0, equal_nan=True)
    assert got[0, 0, 0] == 2.0 and np.isnan(got[:, 1:3, 0]).all() and (got[:, 3, :] == 98.0).all()


def test_rafterydiag_too_few_samples_warns(mamba):
    class NoDevice(hr.HostShard):
        def chain_raftery(self, q):
            raise AssertionError("no device call when nmin > n")

    sh = NoDevice(hr.input_b()[:, :, :3])
    with pytest.warns(UserWarning, match="At least 3746 samples are needed for specified q, r, and s") as rec:
        got = mamba.rafterydiag(sh)
    assert len(rec) == 1
    assert (got[:, 3, :] == 3746.0).all() and np.isnan(np.delete(got, 3, axis=1)).all()
    assert hr.rafterydiag(sh.d[:, 0, 0])[0][3] == 3746.0
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(AssertionError):        # enough samples: the partials are asked for
            mamba.rafterydiag(NoDevice(hr.input_c()[:, :, :2]), Q, R, S)


def test_python_argument_errors(mamba):
    sh = _shard()
    with pytest.raises(mamba.ArgumentError, match="at least 10 iterations"):
        mamba.heideldiag(hr.HostShard(sh.d[:9]))
    with pytest.raises(mamba.ArgumentError, match="unsupported mcse method"):
        mamba.heideldiag(sh, etype="spectral")
    with pytest.raises(mamba.ArgumentError, match="iterations are < 200 and batch size is > 15"):
        mamba.heideldiag(sh, etype="bm")                          # the second half: 30 draws
    for kw, msg in [(dict(q=0.0), "q is not in \\(0, 1\\)"), (dict(q=1.0), "q is not in"),
                    (dict(s=0.0), "s is not in \\(0, 1\\)"), (dict(s=1.2), "s is not in"),
                    (dict(r=0.0), "r must be positive"), (dict(eps=-1.0), "eps must be positive")]:
        with pytest.raises(mamba.ArgumentError, match=msg):
            mamba.rafterydiag(sh, **kw)
    c = mamba.Chains(sh.d, ["a", "b", "c"], 1, 1, np.arange(1, 9))
    for call in (c.heideldiag, c.rafterydiag, c.cor):
        with pytest.raises(mamba.ArgumentError):                  # no engine behind these chains
            call()


def _gelman_sums(psi):
    """The sums as mamba.jl_amd/gelman.py gelmandiag builds them."""
    n, p, m = psi.shape
    means = psi.mean(0)
    S2 = np.einsum("ijk,ilk->jlk", psi - means, psi - means) / (n - 1)
    phi = means.T
    s2 = np.stack([np.diag(S2[:, :, k]) for k in range(m)])
    return np.concatenate([[m], phi.sum(0), (phi.T @ phi).ravel(), S2.sum(2).ravel(),
                           (s2**2).sum(0), (s2 * phi).sum(0), (s2 * phi**2).sum(0)])


def test_cor_from_sums(mamba):
    rng = np.random.default_rng(11)
    v = rng.normal(size=(50, 3, 7))
    v[:, 1] += 0.7 * v[:, 0] + rng.normal(size=7)[None, :]        # correlated, chain means apart
    v[:, 2] -= 0.2 * v[:, 1]
    pooled = v.transpose(0, 2, 1).reshape(-1, 3)
    want = np.corrcoef(pooled, rowvar=False)
    got = mamba.cor_from_sums(_gelman_sums(v), 50, 3)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(hr.cor(v), want, rtol=0, atol=1e-12)
    assert (np.diag(got) == 1.0).all()
    # two shards' sums add up to the whole's (the sum all-reduce), up to the common shift
    parts = _gelman_sums(v[:, :, :3]) + _gelman_sums(v[:, :, 3:])
    np.testing.assert_allclose(mamba.cor_from_sums(parts, 50, 3), want, rtol=0, atol=1e-12)
