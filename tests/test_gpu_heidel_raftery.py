"""heideldiag, rafterydiag and cor on the device (diag.hip through mmb_chain_cvm /
mmb_chain_mcse_from / mmb_chain_raftery, gr.hip through mmb_gr_partials) against the restatement
tests/heidel_raftery_ref.py, on uploaded draws (inputs A, B, C of that module) and on sampler
output.

Tolerances.  Means: tests/test_gpu_diag.py's bound, atol 1e-10 sqrt(gamma0) + rtol 1e-10.  W, mcse,
halfwidth: rtol 1e-8, the project's bound for derived per-chain figures; the mcse bound needs
well-conditioned windows (value >= 0.5 gamma0, every break decision >= 1e-8 gamma0 from zero).  The
Raftery-Lewis threshold, kthin, ntest and counts are exact; bic rtol 1e-9 + atol 1e-9 (its two
logarithms are the device's).  Discrete outcomes (which window converges, Test, where the thinning
loop stops) are exact, which needs every decision to be clear on the reference: each test asserts,
for every series (properties of the inputs, nothing is masked), that each p-value tested is at
least 1e-6 from alpha (I = W / S0 carries about 4e-8 relative error and |dp / dlnI| < 1), the
halfwidth ratio at least 1e-6 relative from eps, and every |bic| at least 1e-9.  Rounded p-values
agree within one unit of the fourth decimal and are equal in more than 99 % of the series."""
import functools
import warnings

import numpy as np
import pytest

import heidel_raftery_ref as hr
import test_gpu_diag as tgd

pytestmark = pytest.mark.gpu

Q, R, S = 0.1, 0.05, 0.9            # Nmin 98
INPUTS = {"A": hr.input_a, "B": hr.input_b, "C": hr.input_c, "n19": hr.input_n19}


@functools.lru_cache(maxsize=None)
def draws(name):
    v = INPUTS[name]()
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def heidel_ref(name, etype):
    return hr.heideldiag_chains(draws(name), etype=etype)


@functools.lru_cache(maxsize=None)
def raftery_ref(name, q):
    return hr.window_raftery(draws(name), q)


@pytest.fixture(scope="module")
def engines(mamba):
    """One engine per input, its draws uploaded once: name -> (draws, engine, Chains)."""
    made = {}

    def get(name, start=1, thin=1):
        if name not in made:
            v = draws(name)
            m, eng = tgd._uploaded(mamba, v)
            made[name] = (v, m, eng)
        v, m, eng = made[name]
        return v, eng, mamba.Chains(v, m.monitor_names, start, thin, np.arange(1, v.shape[2] + 1), m, eng)

    return get


def check_means(got, ref, g0):
    assert np.all(np.abs(got - ref) <= 1e-10 * np.sqrt(g0) + 1e-10 * np.abs(ref))


@pytest.mark.parametrize("name", ["A", "B", "n19", "C"])
def test_chain_cvm(engines, name):
    """Every candidate window of the diagnostic in one call: 5 starts (A, C), 6 (B) and the 9 of
    n = 19, which take the wide instantiation of the kernel."""
    v, eng, _ = engines(name)
    n = v.shape[0]
    starts, _ = hr.heidel_starts(n)
    assert len(starts) == {"A": 5, "B": 6, "n19": 9, "C": 5}[name]
    got = eng.chain_cvm(starts)
    ref = hr.window_cvm(v, starts)
    assert got.shape == ref.shape == (v.shape[2], 3, len(starts), 2)
    for q, s in enumerate(starts):
        check_means(got[:, :, q, 0], ref[:, :, q, 0], v[s:].var(axis=0).T)
    np.testing.assert_allclose(got[:, :, :, 1], ref[:, :, :, 1], rtol=1e-8, atol=0)
    if name == "C":                                  # the chain that never moved
        assert (got[0, :, :, 1] == 0.0).all() and (got[0, :, :, 0] == 1.5).all()
    # a single start, and starts that are no multiples of the unroll
    sub = [3, n // 2]
    np.testing.assert_allclose(eng.chain_cvm(sub[:1])[:, :, 0, 1], hr.window_cvm(v, sub[:1])[:, :, 0, 1], rtol=1e-8)
    np.testing.assert_allclose(eng.chain_cvm(sub)[:, :, :, 1], hr.window_cvm(v, sub)[:, :, :, 1], rtol=1e-8)


@pytest.mark.parametrize("etype", tgd.ETYPES)
def test_chain_mcse_from_equal_starts(engines, etype):
    """Equal starts: the bits of mmb_chain_mcse."""
    v, eng, _ = engines("A")
    n, _, K = v.shape
    for i0 in (0, 160, 199):
        got = eng.chain_mcse_from(np.full((K, 3), i0), n, etype, 10)
        np.testing.assert_array_equal(got, eng.chain_mcse(i0, n, etype, 10))


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("etype", tgd.ETYPES)
def test_chain_mcse_from_mixed_starts(engines, name, etype):
    """A start per series: the windows the diagnostic chooses (every candidate occurs)."""
    v, eng, _ = engines(name)
    n = v.shape[0]
    i0 = heidel_ref(name, "imse")[1]["start"].T.astype(np.int64)             # K x p
    assert set(np.unique(i0)) == set(hr.heidel_starts(n)[0])
    ref, ratio, margin = hr.window_mcse_from(v, i0, n, etype, 5)
    print(f"{name} {etype}: value/gamma0 >= {np.nanmin(ratio):.3g}, closest decision {margin.min():.3g} gamma0")
    assert tgd.well_conditioned(ratio, margin).all()
    tgd.check_mcse(eng.chain_mcse_from(i0, n, etype, 5), ref)


@pytest.mark.parametrize("name,q", [("A", Q), ("C", Q), ("B", 0.25)])
def test_chain_raftery(engines, name, q):
    """q = 0.1 on 400 draws interpolates between two order statistics (C: with ties at the
    threshold); q = 0.25 on the 57 draws of B hits index 15 exactly."""
    v, eng, _ = engines(name)
    ref, least = raftery_ref(name, q)
    print(f"{name}: smallest |bic| {least.min():.3g}, kthin {np.unique(ref[:, :, 1], return_counts=True)}")
    assert (least >= 1e-9).all() and not np.isnan(ref).any()
    if q == Q:
        assert set(np.unique(ref[:, :, 1])) == {1.0, 2.0, 3.0}
    else:
        assert 1.0 + (v.shape[0] - 1) * q == 15.0
    got = eng.chain_raftery(q)
    np.testing.assert_array_equal(got[:, :, :7], ref[:, :, :7])
    np.testing.assert_allclose(got[:, :, 7], ref[:, :, 7], rtol=1e-9, atol=1e-9)


def test_chain_raftery_runs_out(mamba):
    """Series whose thinned sequence drops below 3 elements before bic turns negative (the
    reference: DomainError) get NaN next to chains that stop at once."""
    v = np.random.default_rng(3).normal(size=(5, 3, 70))
    v[:, :, 1] = np.array([0.0, 0.0, 5.0, 5.0, 0.0])[:, None]
    m, eng = tgd._uploaded(mamba, v)
    ref, least = hr.window_raftery(v, 0.5)
    assert np.isnan(ref[1, :, 1]).all() and (ref[1, :, 2] == 2.0).all() and not np.isnan(ref[:, :, 1]).all()
    # the crafted chain: g2 = 4 log 2 against 2 log 3, then at kthin = 2 one triple is left, which
    # fits exactly: bic = 2 log 1 - 2 log 1 = 0 on both sides, as for every series that gets there.
    # A bic of exactly 0 arises in no other way; the others are clear of zero
    assert ((least >= 1e-9) | (least == 0.0)).all() and (least == 0.0).any() and (least >= 1e-9).any()
    got = eng.chain_raftery(0.5)
    np.testing.assert_array_equal(got[:, :, :7], ref[:, :, :7])
    np.testing.assert_array_equal(np.isnan(got[:, :, 7]), np.isnan(ref[:, :, 7]))
    np.testing.assert_allclose(got[:, :, 7], ref[:, :, 7], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("name,start,thin", [("A", 1, 1), ("C", 101, 2)])
def test_rafterydiag(engines, name, start, thin):
    v, eng, sim = engines(name, start, thin)
    ref, least = hr.rafterydiag_chains(v, Q, R, S, start=start, thin=thin)
    assert (least >= 1e-9).all() and (ref[:, 3, :] == 98.0).all()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = sim.rafterydiag(Q, R, S)
    assert got.shape == (3, 5, v.shape[2])
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0)
    if name == "C":                                  # the constant chain: kthin 1 (x thin), the rest NaN
        assert (got[:, 0, 0] == thin).all() and np.isnan(got[:, [1, 2, 4], 0]).all()
        assert (np.unique(got[:, 0, :]) == [2.0, 4.0, 6.0]).all()


def test_rafterydiag_too_few_samples(engines):
    v, eng, sim = engines("B")
    with pytest.warns(UserWarning, match="At least 98 samples are needed for specified q, r, and s"):
        got = sim.rafterydiag(Q, R, S)
    assert (got[:, 3, :] == 98.0).all() and np.isnan(np.delete(got, 3, axis=1)).all()


def check_heidel(v, got, ref, side, start, nonconv=None):
    """The Heidelberger-Welch comparison of the module docstring; `side` are the reference's
    conditioning figures."""
    n = v.shape[0]
    print(f"closest p-value to alpha {side['pgap'].min():.3g}, halfwidth ratio to eps {side['hwgap'].min():.3g}, "
          f"value/gamma0 >= {np.nanmin(side['value_ratio']):.3g}, closest decision {side['margin'].min():.3g} gamma0, "
          f"{int((ref[:, 1, :] == 0).sum())} series not converged, burn-ins {np.unique(ref[:, 0, :])}")
    assert (side["pgap"] >= 1e-6).all() and (side["hwgap"] >= 1e-6).all()
    assert tgd.well_conditioned(side["value_ratio"], side["margin"]).all()
    if nonconv is not None:
        starts, i_final = hr.heidel_starts(n)
        assert int((ref[:, 1, :] == 0).sum()) == nonconv
        assert set(np.unique(ref[:, 0, :])) == {s + start - 1 for s in starts} | {i_final + start - 2}
    assert got.shape == ref.shape
    np.testing.assert_array_equal(got[:, [0, 1, 5], :], ref[:, [0, 1, 5], :])
    g0 = np.array([[v[int(side["start"][j, k]):, j, k].var() for k in range(v.shape[2])] for j in range(3)])
    check_means(got[:, 3, :], ref[:, 3, :], g0)
    np.testing.assert_array_equal(np.isnan(got[:, 4, :]), np.isnan(ref[:, 4, :]))
    np.testing.assert_allclose(got[:, 4, :], ref[:, 4, :], rtol=1e-8, atol=0)
    np.testing.assert_allclose(got[:, 2, :], ref[:, 2, :], rtol=0, atol=1.001e-4)
    assert (got[:, 2, :] == ref[:, 2, :]).mean() > 0.99


@pytest.mark.parametrize("name,etype,nonconv", [("A", "imse", 5), ("A", "ipse", 3), ("B", "imse", 2), ("B", "ipse", 2)])
def test_heideldiag(engines, name, etype, nonconv):
    v, eng, sim = engines(name)
    ref, side = heidel_ref(name, etype)
    check_heidel(v, sim.heideldiag(etype=etype), ref, side, 1, nonconv)


def test_heideldiag_constant_chain(engines):
    """S0 = 0 and W = 0 exactly on the device too: p-value NaN, not converged, halfwidth 0, Test 1."""
    v, eng, sim = engines("C", 101, 2)
    got = sim.heideldiag()
    for j in range(3):
        np.testing.assert_array_equal(got[j, :, 0], [201 + 101 - 2, 0.0, np.nan, 1.5, 0.0, 1.0])
    assert not np.isnan(got[:, 2, 1:]).any()


def test_cor(engines):
    """The pooled correlation from the Gelman-Rubin sums (each within rtol 1e-10): absolute, an
    off-diagonal entry can be near zero."""
    v, eng, sim = engines("A")
    got = sim.cor()
    np.testing.assert_allclose(got, hr.cor(v), rtol=0, atol=1e-9)
    assert (np.diag(got) == 1.0).all() and np.array_equal(got, got.T)


def test_end_to_end_on_sampler_output(mamba):
    d, sim = tgd._sampled(mamba, 500, 1)
    assert d.shape == (400, 3, 96) and sim.start == 101
    ref, side = hr.heideldiag_chains(d, start=101)
    check_heidel(d, sim.heideldiag(), ref, side, 101)
    rref, least = hr.rafterydiag_chains(d, Q, R, S, start=101)
    print(f"smallest |bic| {least.min():.3g}")
    assert (least >= 1e-9).all()
    got = sim.rafterydiag(Q, R, S)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(rref))
    np.testing.assert_allclose(got, rref, rtol=1e-12, atol=0)
    np.testing.assert_allclose(sim.cor(), hr.cor(d), rtol=0, atol=1e-9)


def test_abi_error_cases(mamba):
    m, eng = tgd._engine(mamba, 5)
    for call in (lambda: eng.chain_cvm([0]), lambda: eng.chain_mcse_from(np.zeros((5, 3)), 2, "imse"),
                 lambda: eng.chain_raftery(0.1)):
        with pytest.raises(RuntimeError, match=r"error -4 .*no device-kept draws"):
            call()
    eng.set_draws(tgd.tiny_draws(30)[:, :, :1].repeat(5, axis=2))
    for bad in ([-1], [30], [0, 31], [5, 5], [6, 5]):
        with pytest.raises(RuntimeError, match="error -1 .*(start|strictly increasing)"):
            eng.chain_cvm(bad)
    for ns in (0, 17):
        with pytest.raises(RuntimeError, match="error -1 .*nstarts"):
            eng.chain_cvm(list(range(ns)))
    assert eng.chain_cvm(list(range(16))).shape == (5, 3, 16, 2)
    for q in (0.0, 1.0, -0.5, float("nan")):
        with pytest.raises(RuntimeError, match="error -1 .*q is not in"):
            eng.chain_raftery(q)
    i0 = np.zeros((5, 3), dtype=np.int64)
    for bad in (30, 31, -1):                          # a start at or beyond i1, or before the draws
        i0[3, 2] = bad
        with pytest.raises(RuntimeError, match=r"error -1 .*window.*\(chain 3, param 2\)"):
            eng.chain_mcse_from(i0, 30, "imse")
    i0[3, 2] = 29
    with pytest.raises(RuntimeError, match=r"error -1 .*lags must be less.*\(chain 3, param 2\)"):
        eng.chain_mcse_from(i0, 30, "ipse")
    i0[3, 2] = 11
    with pytest.raises(RuntimeError, match=r"error -1 .*iterations are < 20 and batch size is > 9.*\(chain 3, param 2\)"):
        eng.chain_mcse_from(i0, 30, "bm", 10)
    with pytest.raises(RuntimeError, match="error -1 .*unsupported mcse method"):
        eng.chain_mcse_from(i0, 30, 7)
    with pytest.raises(RuntimeError, match="error -1 .*window"):
        eng.chain_mcse_from(i0, 31, "imse")
    with pytest.raises(mamba.ArgumentError, match="window starts must be 5 x 3"):
        eng.chain_mcse_from(np.zeros((3, 5)), 30, "imse")
    eng.set_draws(tgd.tiny_draws(2)[:, :, :1].repeat(5, axis=2))
    with pytest.raises(RuntimeError, match="error -1 .*3 <= kept draws"):
        eng.chain_raftery(0.5)
