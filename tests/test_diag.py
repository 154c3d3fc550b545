"""Per-chain diagnostics (autocor, changerate, gewekediag, mcse) without a GPU: the C ABI's
host-side validation, the Python argument errors of the reference, the restatement
tests/diag_ref.py pinned by closed forms, and the host formulas of mamba.jl_amd/diag.py fed by an
engine-shaped host shard (diag_ref.HostDiagShard).  The kernels are checked in
tests/test_gpu_diag.py."""
import ctypes as C
import math

import numpy as np
import pytest

import diag_ref


def test_entry_points_reject_null(mamba):
    lib = mamba.abi.lib()
    out = np.zeros(8)
    lags = (C.c_int64 * 1)(1)
    cnt = (C.c_int64 * 4)()
    assert lib.mmb_set_draws(None, mamba.abi.dptr(out), 2) == -1
    assert lib.mmb_chain_autocov(None, 0, 4, 1, lags, mamba.abi.dptr(out)) == -1
    assert lib.mmb_chain_mcse(None, 0, 4, mamba.abi.MMB_MCSE_IMSE, 100, mamba.abi.dptr(out)) == -1
    assert lib.mmb_change_counts(None, cnt) == -1
    assert b"null" in lib.mmb_last_error(None)
    a = mamba.abi
    assert (a.MMB_DIAG_MAX_LAGS, a.MMB_MCSE_FIELDS, a.MMB_MCSE_BM, a.MMB_MCSE_IMSE, a.MMB_MCSE_IPSE) == (16, 4, 0, 1, 2)
    assert a.MMB_ABI_VERSION == 10


def _shard(n=60, p=2, m=3, seed=0):
    return diag_ref.HostDiagShard(np.random.default_rng(seed).normal(size=(n, p, m)).cumsum(0))


def test_python_argument_errors(mamba):
    sh = _shard()
    for kw, msg in [(dict(first=0.0), "first is not in \\(0, 1\\)"), (dict(first=1.0), "first is not in"),
                    (dict(last=0.0), "last is not in \\(0, 1\\)"), (dict(last=1.5), "last is not in"),
                    (dict(first=0.6, last=0.5), "first and last proportions overlap")]:
        with pytest.raises(mamba.ArgumentError, match=msg):
            mamba.gewekediag(sh, **kw)
    with pytest.raises(mamba.ArgumentError, match="lags do not correspond to thinning interval"):
        mamba.autocor(sh, lags=(2, 5), thin=2, relative=False)
    with pytest.raises(mamba.ArgumentError, match="lags must be less than the sample length"):
        mamba.autocor(sh, lags=(1, 60))
    with pytest.raises(mamba.ArgumentError, match="lags must be less than the sample length"):
        mamba.autocor(sh, lags=(30,), thin=2)                    # relative: index lag 60
    with pytest.raises(mamba.ArgumentError, match="iterations are < 200 and batch size is > 3"):
        mamba.gewekediag(sh, etype="bm")                         # first window: 6 draws
    with pytest.raises(mamba.ArgumentError, match="iterations are < 200 and batch size is > 30"):
        mamba.diag.mcse(sh, "bm")
    with pytest.raises(mamba.ArgumentError, match="unsupported mcse method"):
        mamba.diag.mcse(sh, "spectral")
    c = mamba.Chains(sh.d, ["a", "b"], 1, 1, np.arange(1, 4))
    for call in (c.autocor, c.changerate, c.gewekediag, c.mcse, c.upload):
        with pytest.raises(mamba.ArgumentError):                 # no engine behind these chains
            call()


def test_index_lags(mamba):
    assert mamba.diag.index_lags((1, 5, 10, 50), 2, True) == [2, 10, 20, 100]
    assert mamba.diag.index_lags((2, 10), 2, False) == [2, 10]
    vals, labels = mamba.autocor(_shard(), lags=(1, 5), thin=2)
    assert labels == ["Lag 2", "Lag 10"] and vals.shape == (2, 2, 3)


@pytest.mark.parametrize("n,w1,w2", [(10, (0, 1), (5, 10)), (200, (0, 20), (100, 200)),
                                     (400, (0, 40), (200, 400)), (401, (0, 40), (201, 401))])
def test_geweke_windows(mamba, n, w1, w2):
    """x[1:round(Int, 0.1 n)] and x[round(Int, n - 0.5 n + 1):n] (gewekediag.jl:13-14), 0-based."""
    assert mamba.geweke_windows(n) == (w1, w2)
    assert diag_ref.geweke_windows(n) == (w1, w2)


# ---- the restatement, pinned by closed forms ---------------------------------------------
def test_ref_two_points():
    """x = (a, b): z = -+d/2, gamma(0) = d^2/4, gamma(1) = -d^2/8; m = 0 so no loop.
    IMSE value = -g0 + 2 (g0 + g1) = 0, IPSE value = g0 + 2 g1 = 0: mcse 0 for both."""
    x = np.array([1.0, 3.0])
    assert diag_ref.autocov(x, [0, 1]) == [1.0, -0.5]
    for f in (diag_ref.mcse_imse, diag_ref.mcse_ipse):
        r = f(x)
        assert (r["mcse"], r["mean"], r["gamma0"], r["terms"], r["margin"]) == (0.0, 2.0, 1.0, 0, math.inf)
    with pytest.raises(ValueError, match="lags must be less"):
        diag_ref.autocov(x, [2])


def test_ref_alternating_series_is_nan():
    """x_t = (-1)^t, n = 7: mean 1/7, every pair sum gamma(2i) + gamma(2i+1) is positive and
    small, and value = -gamma(0) + 2 sum(pairs) is negative (-0.214 gamma(0)): the reference's
    sqrt throws, the restatement gives NaN."""
    x = np.array([(-1.0) ** t for t in range(7)])
    g = diag_ref.autocov(x, range(7))
    z = x - 1.0 / 7.0
    for l in range(7):
        assert g[l] == pytest.approx(sum(z[t] * z[t + l] for t in range(7 - l)) / 7.0, rel=1e-14)
    for f in (diag_ref.mcse_imse, diag_ref.mcse_ipse):
        r = f(x)
        assert math.isnan(r["mcse"]) and r["terms"] == 2
        assert r["value_ratio"] == pytest.approx(-0.2142857142857, rel=1e-9)
        assert r["margin"] == pytest.approx(min(abs(g[2] + g[3]), abs(g[4] + g[5])) / g[0], rel=1e-12)


def test_ref_constant_series():
    x = np.full(9, 1.5)
    assert diag_ref.autocov(x, [0, 1, 8]) == [0.0, 0.0, 0.0]
    for et in ("imse", "ipse"):
        r = diag_ref.mcse(x, et)
        assert r["mcse"] == 0.0 and r["mean"] == 1.5 and r["terms"] == 0
    assert diag_ref.mcse_bm(np.full(40, 1.5), 10)["mcse"] == 0.0
    v = np.full((30, 1, 1), 1.5)
    assert np.isnan(diag_ref.autocor(v, (1, 5))[0]).all()
    vals, zs, _, _ = diag_ref.gewekediag(v)
    assert np.isnan(zs).all() and np.isnan(vals).all()
    np.testing.assert_array_equal(diag_ref.change_counts(v), [0, 0])


def test_ref_bm_against_numpy():
    x = np.random.default_rng(3).normal(size=95).cumsum()
    mb = x[:90].reshape(9, 10).mean(1)
    assert diag_ref.mcse_bm(x, 10)["mcse"] == pytest.approx(mb.std(ddof=1) / 3.0, rel=1e-12)
    with pytest.raises(ValueError, match="iterations are < 100 and batch size is > 47"):
        diag_ref.mcse_bm(x, 50)


def test_ref_changerate_by_hand():
    v = np.zeros((4, 2, 2))
    v[:, 0, 0] = [1, 1, 2, 2]      # 1 change
    v[:, 1, 0] = [0, 3, 3, 3]      # 1 change, at another step
    v[:, 0, 1] = [5, 6, 7, 8]      # 3 changes
    np.testing.assert_array_equal(diag_ref.change_counts(v), [4, 1, 5])
    np.testing.assert_array_equal(diag_ref.changerate(v), np.round(np.array([4, 1, 5]) / 6.0, 3))


# ---- the host formulas over an engine-shaped shard -----------------------------------------
def test_host_formulas_against_the_restatement(mamba):
    sh = _shard(n=120, p=2, m=4, seed=5)
    got, labels = mamba.autocor(sh, lags=(1, 5, 10, 50))
    ref, rlabels = diag_ref.autocor(sh.d, (1, 5, 10, 50))
    assert labels == rlabels == ["Lag 1", "Lag 5", "Lag 10", "Lag 50"]
    np.testing.assert_allclose(got, ref, rtol=1e-12)
    many = tuple(range(1, 21))                                   # more than MMB_DIAG_MAX_LAGS: two calls
    np.testing.assert_allclose(mamba.autocor(sh, lags=many)[0], diag_ref.autocor(sh.d, many)[0], rtol=1e-12)
    for et in ("imse", "ipse", "bm"):
        vals, zs, _, _ = diag_ref.gewekediag(sh.d, etype=et, size=5)
        np.testing.assert_allclose(mamba.geweke_z(sh, etype=et, batch_size=5), zs, rtol=1e-12)
        np.testing.assert_array_equal(mamba.gewekediag(sh, etype=et, batch_size=5), vals)
        np.testing.assert_allclose(mamba.diag.mcse(sh, et, 5), diag_ref.window_mcse(sh.d, 0, 120, et, 5)[0][:, :, 2].T,
                                   rtol=1e-12)
    np.testing.assert_array_equal(mamba.changerate_sharded(sh), diag_ref.changerate(sh.d))


def test_changerate_two_shards_equal_one(mamba):
    d = np.random.default_rng(7).integers(0, 3, size=(12, 3, 9)).astype(float)
    shards = [diag_ref.HostDiagShard(d[:, :, :4]), diag_ref.HostDiagShard(d[:, :, 4:])]
    parts = [np.concatenate([s.change_counts().astype(float), [float(s.K)]]) for s in shards]
    total = parts[0] + parts[1]

    def allreduce_sum(v):                                        # what every rank sees after the sum
        assert any(np.array_equal(v, q) for q in parts)
        return total

    want = diag_ref.changerate(d)
    for s in shards:
        np.testing.assert_array_equal(mamba.changerate_sharded(s, allreduce_sum), want)
    np.testing.assert_array_equal(mamba.changerate_sharded(diag_ref.HostDiagShard(d)), want)
