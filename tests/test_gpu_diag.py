"""Per-chain diagnostics on the device (diag.hip through mmb_set_draws / mmb_chain_autocov /
mmb_chain_mcse / mmb_change_counts) against the restatement tests/diag_ref.py.

Tolerances (those of tests/test_summary.py:108-109): mean atol 1e-10 sqrt(gamma0) + rtol 1e-10;
gamma(l) atol 1e-10 gamma0 (so near-zero autocovariances are covered); mcse and z rtol 1e-8.
The mcse / z bound needs a well-conditioned series: value >= 0.5 gamma0 and every
`Ghat > 0 || break` decision at least 1e-8 gamma0 from zero (100x the gamma tolerance, so a
reordered sum cannot flip a break).  Each test asserts these conditions on the reference for every
one of its series (they are properties of the inputs, nothing is masked); tests that craft
negative values on purpose ask instead that the value is clearly negative (<= -1e-6 gamma0, far
beyond the summed gamma tolerance of a few hundred terms), where NaN is expected.  NaN patterns
must agree exactly; change counts are integers and compared exactly."""
import os
import sys

import numpy as np
import pytest

import diag_ref

pytestmark = pytest.mark.gpu

ETYPES = ("bm", "imse", "ipse")


def _summary_ref():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import summary_ref
    return summary_ref


def _engine(mamba, K, seed=3):
    m = mamba.line()
    m.setinputs(mamba.model.LINE_DATA)
    m.setsamplers([mamba.AMWG(["beta", "s2"], 1.0)])
    eng = mamba.Engine(m)
    eng.init_chains(mamba.model.line_init_matrix(K, seed=seed), seed=7)
    return m, eng


def _uploaded(mamba, value):
    m, eng = _engine(mamba, value.shape[2])
    eng.set_draws(value)
    assert eng.num_kept() == value.shape[0]
    return m, eng


def ar1(n, K, seed=1, phis=(0.3, 0.6, 0.9), shift=(0.0, 25.0, -1000.0)):
    """n x 3 x K AR(1) series x_t = phi x_{t-1} + e_t, one phi per param, on distinct levels."""
    e = np.random.default_rng(seed).normal(size=(n, 3, K))
    x = np.empty_like(e)
    ph = np.asarray(phis)[:, None]
    x[0] = e[0]
    for t in range(1, n):
        x[t] = ph * x[t - 1] + e[t]
    return x + np.asarray(shift)[None, :, None]


def edge_draws(n=301, K=65, seed=2):
    """Chain 0 constant 1.5, chain 1 alternating +-1 (n odd: mean 1/n, value clearly negative),
    the rest AR(1)."""
    x = ar1(n, K, seed, phis=(0.5, 0.5, 0.5), shift=(0.0, 3.0, -7.0))
    x[:, :, 0] = 1.5
    x[:, :, 1] = ((-1.0) ** np.arange(n))[:, None]
    return x


def tiny_draws(n, seed=4):
    """n x 3 x 3 normal draws on multiples of 1/256 (sums of two and their halves are exact)."""
    x = np.random.default_rng(seed).normal(size=(n, 3, 3)) + np.array([0.0, 10.0, -3.0])[None, :, None]
    return np.round(x * 256.0) / 256.0


def well_conditioned(ratio, margin, allow_negative=False):
    """The two conditions of the module docstring, per series.  A constant series (gamma0 = 0:
    ratio NaN, no decision) is exact on both sides and passes."""
    ok = (ratio >= 0.5) | np.isnan(ratio)
    if allow_negative:
        ok |= ratio <= -1e-6
    return ok & (margin >= 1e-8)


def check_autocov(got, ref):
    g0 = ref[:, :, 1]
    assert np.all(np.abs(got[:, :, 0] - ref[:, :, 0]) <= 1e-10 * np.sqrt(g0) + 1e-10 * np.abs(ref[:, :, 0]))
    assert np.all(np.abs(got[:, :, 1:] - ref[:, :, 1:]) <= 1e-10 * g0[:, :, None])


def check_mcse(got, ref):
    check_autocov(got[:, :, :2], ref[:, :, :2])
    np.testing.assert_array_equal(np.isnan(got[:, :, 2]), np.isnan(ref[:, :, 2]))
    np.testing.assert_allclose(got[:, :, 2], ref[:, :, 2], rtol=1e-8, atol=0)
    np.testing.assert_array_equal(got[:, :, 3], ref[:, :, 3])


@pytest.mark.parametrize("K", [96, 1])
def test_set_draws_round_trip(mamba, K):
    """Uploaded draws come back bit for bit and the existing device summaries run on them."""
    sr = _summary_ref()
    v = np.random.default_rng(K).normal(size=(7, 3, K)) * np.array([1.0, 30.0, 0.01])[None, :, None] + 4.0
    m, eng = _engine(mamba, K)
    sim = mamba.Chains(v, m.monitor_names, 1, 1, np.arange(1, K + 1), m, eng)
    with pytest.raises(mamba.ArgumentError):       # nothing on the device yet
        sim.summarystats(3)
    assert sim.upload() is sim and eng.num_kept() == 7
    np.testing.assert_array_equal(eng.draws(), v)
    got, ref = sim.summarystats(3), sr.summarystats(v, 3)
    np.testing.assert_allclose(got[:, :4], ref[:, :4], rtol=1e-10)
    np.testing.assert_allclose(got[:, 4], ref[:, 4], rtol=1e-8)
    eng.set_draws(v[:2])                           # a shorter upload replaces the window
    np.testing.assert_array_equal(eng.draws(), v[:2])
    with pytest.raises(mamba.ArgumentError):
        eng.set_draws(v[:, :2, :])


@pytest.fixture(scope="module")
def ar1_engine(mamba):
    v = ar1(400, 96, seed=1)
    m, eng = _uploaded(mamba, v)
    return v, eng


@pytest.mark.parametrize("i0,i1,lags", [(0, 400, (1, 5, 10, 50)), (0, 40, (1, 5, 10)), (0, 40, (1, 39)),
                                        (200, 400, (1, 5, 10, 50)), (200, 400, tuple(range(1, 17)))])
def test_autocov_crafted_ar1(ar1_engine, i0, i1, lags):
    """gamma at a lag list in one sweep; 39 = n_w - 1 is the longest lag a window of 40 has; 16
    lags is MMB_DIAG_MAX_LAGS (the wide instantiation of the kernel)."""
    v, eng = ar1_engine
    check_autocov(eng.chain_autocov(i0, i1, lags), diag_ref.window_autocov(v, i0, i1, lags))


@pytest.mark.parametrize("i0,i1", [(0, 400), (0, 40), (200, 400)])
@pytest.mark.parametrize("etype", ETYPES)
def test_mcse_crafted_ar1(ar1_engine, etype, i0, i1):
    v, eng = ar1_engine
    ref, ratio, margin = diag_ref.window_mcse(v, i0, i1, etype, 10)
    print(f"{etype} [{i0},{i1}): value/gamma0 >= {ratio.min():.3g}, closest decision {margin.min():.3g} gamma0, "
          f"up to {int(ref[:, :, 3].max())} terms")
    assert well_conditioned(ratio, margin).all()
    check_mcse(eng.chain_mcse(i0, i1, etype, 10), ref)


@pytest.mark.parametrize("n", [2, 3, 4, 5])
def test_tiny_windows(mamba, n):
    """m = div(n - 2, 2) = 0, 0, 1, 1: no loop, or a single pair.  With n even and every pair
    added, value is gamma(0) + 2 sum_{l>=1} gamma(l) = (sum z)^2 / n = 0 in exact arithmetic; the
    draws are multiples of 1/256, so for n = 2 and 4 the mean (a division by 2 or 4), z, the
    products and their sums are all exact on both sides and such a value is 0.0 (mcse 0.0) on both.
    Otherwise value is a sum of at most 6 autocovariances of at most 5 products each, within
    1e-14 gamma0 of the reference's whatever the order, so its sign (NaN or not) is beyond doubt,
    and mcse within rtol 1e-8, once |value| >= 1e-6 gamma0."""
    v = tiny_draws(n)
    m, eng = _uploaded(mamba, v)
    for etype in ("imse", "ipse"):
        ref, ratio, margin = diag_ref.window_mcse(v, 0, n, etype)
        print(f"n={n} {etype}: value/gamma0 {np.sort(ratio.ravel())}, closest decision {margin.min():.3g}")
        assert (margin >= 1e-8).all()
        assert (ratio == 0.0).all() if n == 2 else (np.abs(ratio) >= 1e-6).all() if n % 2 else \
            ((ratio == 0.0) | (np.abs(ratio) >= 1e-6)).all()
        np.testing.assert_array_equal(np.isnan(ref[:, :, 2]), ratio < 0)
        check_mcse(eng.chain_mcse(0, n, etype), ref)
    if n > 2:
        check_autocov(eng.chain_autocov(0, n, (1, n - 1)), diag_ref.window_autocov(v, 0, n, (1, n - 1)))


def test_edge_chains(mamba):
    """A chain that never moved (gamma = 0 exactly: mcse 0.0, autocor and z NaN), an alternating
    chain (negative value: NaN where the reference throws) and a partial second wavefront."""
    v = edge_draws()
    n, _, K = v.shape
    m, eng = _uploaded(mamba, v)
    sim = mamba.Chains(v, m.monitor_names, 1, 1, np.arange(1, K + 1), m, eng)
    for etype in ("imse", "ipse"):
        ref, ratio, margin = diag_ref.window_mcse(v, 0, n, etype)
        assert well_conditioned(ratio, margin, allow_negative=True).all()
        assert np.isnan(ref[1, :, 2]).all() and (ref[0, :, 2] == 0.0).all()
        got = eng.chain_mcse(0, n, etype)
        check_mcse(got, ref)
        assert (got[0, :, 2] == 0.0).all() and (got[0, :, 1] == 0.0).all() and (got[0, :, 0] == 1.5).all()
        np.testing.assert_array_equal(sim.mcse(etype), got[:, :, 2].T)
        # odd windows, so the alternating chain's value stays clearly negative in both
        vals, zs, ratio, margin = diag_ref.gewekediag(v, 0.13, 0.49, etype)
        assert well_conditioned(ratio, margin, allow_negative=True).all()
        z = mamba.geweke_z(eng, 0.13, 0.49, etype)
        np.testing.assert_array_equal(np.isnan(z), np.isnan(zs))
        assert np.isnan(z[:, :2]).all() and not np.isnan(z[:, 2:]).any()
        np.testing.assert_allclose(z, zs, rtol=1e-8, atol=0)
    got = eng.chain_mcse(0, n, "bm", 10)
    check_mcse(got, diag_ref.window_mcse(v, 0, n, "bm", 10)[0])
    assert (got[0, :, 2] == 0.0).all()
    ac, labels = sim.autocor(lags=(1, 5, 10, 50))
    rac, _ = diag_ref.autocor(v, (1, 5, 10, 50))
    np.testing.assert_array_equal(np.isnan(ac), np.isnan(rac))
    assert np.isnan(ac[:, :, 0]).all() and not np.isnan(ac[:, :, 1:]).any()
    np.testing.assert_allclose(ac, rac, rtol=0, atol=2e-10)      # gamma(l), gamma0 each within 1e-10 gamma0, |rho| <= 1


@pytest.mark.parametrize("n,K", [(9, 70), (1, 70), (2, 3), (100, 130)])
def test_change_counts(mamba, n, K):
    """Integer-valued draws with many repeats; n = 1 has no transitions; n = 100 runs several
    row ranges and a partial step."""
    v = np.random.default_rng(n + K).integers(0, 3, size=(n, 3, K)).astype(np.float64)
    v[:, 2, ::2] = 5.0                                           # a param that never moves in half the chains
    m, eng = _uploaded(mamba, v)
    ref = diag_ref.change_counts(v)
    np.testing.assert_array_equal(eng.change_counts(), ref)
    if n == 1:
        assert not ref.any()
    else:
        sim = mamba.Chains(v, m.monitor_names, 1, 1, np.arange(1, K + 1), m, eng)
        np.testing.assert_array_equal(sim.changerate(), diag_ref.changerate(v))


def _sampled(mamba, iters, thin):
    m = mamba.line()
    m.setinputs(mamba.model.LINE_DATA)
    m.setsamplers([mamba.AMWG(["beta", "s2"], 1.0)])
    eng = mamba.Engine(m)
    eng.init_chains(mamba.model.line_init_matrix(96, seed=5), seed=11)
    d = eng.run(iters, burnin=100, thin=thin, keep_device=True)
    return d, mamba.Chains(d, m.monitor_names, 100 + thin, thin, np.arange(1, 97), m, eng)


def test_end_to_end_on_sampler_output(mamba):
    d, sim = _sampled(mamba, 500, 1)
    assert d.shape == (400, 3, 96)
    ac, labels = sim.autocor()
    rac, rlabels = diag_ref.autocor(d)
    assert labels == rlabels == ["Lag 1", "Lag 5", "Lag 10", "Lag 50"]
    np.testing.assert_allclose(ac, rac, rtol=0, atol=2e-10)
    np.testing.assert_array_equal(sim.changerate(), diag_ref.changerate(d))
    for etype in ("imse", "ipse"):
        vals, zs, ratio, margin = diag_ref.gewekediag(d, etype=etype)
        print(f"{etype}: value/gamma0 >= {ratio.min():.3g}, closest decision {margin.min():.3g} gamma0")
        assert well_conditioned(ratio, margin).all() and not np.isnan(ratio).any()
        np.testing.assert_allclose(mamba.geweke_z(sim.engine, etype=etype), zs, rtol=1e-8, atol=0)
        got = sim.gewekediag(etype=etype)
        assert got.shape == (3, 2, 96)
        # the rounded figures agree unless z sits within 1e-8 |z| of a rounding boundary
        np.testing.assert_allclose(got, vals, rtol=0, atol=1.001e-3)
        assert (got == vals).mean() > 0.99


def test_end_to_end_thinned_lags(mamba):
    """thin = 2: relative lags (1, 5, 10, 50) are index lags (2, 10, 20, 100) of the kept series
    (stats.jl:5-6); relative=False takes (2, 10) as they are and refuses an odd lag."""
    d, sim = _sampled(mamba, 900, 2)
    assert d.shape == (400, 3, 96)
    ac, labels = sim.autocor()
    rac, rlabels = diag_ref.autocor(d, thin=2)
    assert labels == rlabels == ["Lag 2", "Lag 10", "Lag 20", "Lag 100"]
    np.testing.assert_allclose(ac, rac, rtol=0, atol=2e-10)
    ac2, labels2 = sim.autocor(lags=(2, 10), relative=False)
    assert labels2 == ["Lag 2", "Lag 10"]
    np.testing.assert_array_equal(ac2, ac[:, :2, :])
    with pytest.raises(mamba.ArgumentError, match="lags do not correspond to thinning interval"):
        sim.autocor(lags=(1, 5), relative=False)
    vals, zs, ratio, margin = diag_ref.gewekediag(d)
    print(f"thin 2: value/gamma0 >= {ratio.min():.3g}, closest decision {margin.min():.3g} gamma0")
    assert well_conditioned(ratio, margin).all()
    np.testing.assert_allclose(mamba.geweke_z(sim.engine), zs, rtol=1e-8, atol=0)
    np.testing.assert_array_equal(sim.changerate(), diag_ref.changerate(d))


def test_abi_error_cases(mamba):
    m, eng = _engine(mamba, 5)
    for call in (lambda: eng.chain_autocov(0, 1, ()), lambda: eng.chain_mcse(0, 2, "imse"), eng.change_counts):
        with pytest.raises(RuntimeError, match=r"error -4 .*no device-kept draws"):
            call()
    with pytest.raises(RuntimeError, match="error -1"):
        mamba.abi.check(eng.lib.mmb_set_draws(eng.h, mamba.abi.dptr(np.zeros(15)), 0), eng.h)
    eng.set_draws(tiny_draws(30)[:, :, :1].repeat(5, axis=2))
    for bad in ((5, 5), (6, 5), (-1, 5), (0, 31)):
        with pytest.raises(RuntimeError, match="error -1 .*window"):
            eng.chain_autocov(bad[0], bad[1], (1,))
        with pytest.raises(RuntimeError, match="error -1 .*window"):
            eng.chain_mcse(bad[0], bad[1], "ipse")
    for lags in ((0,), (30,), (1, 10), (-2,)):
        with pytest.raises(RuntimeError, match="error -1 .*lags must be less than the sample length"):
            eng.chain_autocov(0, 10 if lags == (1, 10) else 30, lags)
    with pytest.raises(RuntimeError, match="error -1 .*nlags"):
        eng.chain_autocov(0, 30, tuple(range(1, 18)))
    with pytest.raises(RuntimeError, match="error -1 .*iterations are < 40 and batch size is > 15"):
        eng.chain_mcse(0, 30, "bm", 20)
    with pytest.raises(RuntimeError, match="error -1 .*lags must be less"):
        eng.chain_mcse(3, 4, "imse")
    with pytest.raises(RuntimeError, match="error -1 .*unsupported mcse method"):
        eng.chain_mcse(0, 30, 7)
    assert eng.chain_autocov(0, 30, ()).shape == (5, 3, 2)       # nlags = 0: mean and gamma(0) alone
    assert eng.chain_mcse(0, 30, "bm", 15)[0, 0, 3] == 2.0
