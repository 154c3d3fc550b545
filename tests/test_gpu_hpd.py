"""hpd on the device (hpd.hip through mmb_hpd_collect / mmb_hpd_set_tails / mmb_hpd_gap, thresholds
from mmb_order_hist) against the np.sort restatement tests/hpd_ref.py, on uploaded draws (the
inputs of that module) and on sampler output.  No tolerance anywhere: the device sorts the same
doubles and takes one IEEE subtraction per candidate, so intervals and the index of the first
minimum are compared exactly."""
import functools

import numpy as np
import pytest

import hpd_ref
import test_gpu_diag as tgd

pytestmark = pytest.mark.gpu

ALPHAS = (1e-9, 0.05, 0.3, 0.5, 0.7, 0.999)
CASES = [(nm, a) for nm in ("small", "flat") for a in ALPHAS] + [("big", a) for a in (0.05, 0.5, 0.999)]
SORT_TILE = 4096   # hpd.hip HPD_TILE


@functools.lru_cache(maxsize=None)
def draws(name):
    v = hpd_ref.INPUTS[name]()
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def ref(name, alpha):
    return hpd_ref.hpd(draws(name), alpha)


@pytest.fixture(scope="module")
def engines(mamba):
    """One engine per input, its draws uploaded once: name -> (draws, engine, Chains)."""
    made = {}

    def get(name):
        if name not in made:
            v = draws(name)
            m, eng = tgd._uploaded(mamba, v)
            made[name] = (v, eng, mamba.Chains(v, m.monitor_names, 1, 1, np.arange(1, v.shape[2] + 1), m, eng))
        return made[name]

    return get


@pytest.mark.parametrize("name,alpha", CASES)
def test_chains_hpd(engines, mamba, name, alpha):
    """Chains.hpd equals the reference exactly, and so does the index of the first minimum; big at
    0.999 sorts two tails of about 102698 values: many workgroups, every digit pass."""
    v, eng, ch = engines(name)
    rv, ri = ref(name, alpha)
    vals, labels = ch.hpd(alpha)
    assert labels == mamba.summary.hpd_labels(alpha) and vals.shape == (3, 2)
    np.testing.assert_array_equal(vals, rv)
    got, idx = mamba.summary.hpd_sharded(eng, alpha, return_index=True)
    np.testing.assert_array_equal(got, rv)
    np.testing.assert_array_equal(idx, ri)


def test_hpd_repeatable(engines, mamba):
    """Twice on one engine, a larger request in between: buffers are reused, no stale counts."""
    _, eng, _ = engines("small")
    first = mamba.summary.hpd_sharded(eng, 0.05, return_index=True)
    mamba.summary.hpd_sharded(eng, 0.7)
    again = mamba.summary.hpd_sharded(eng, 0.05, return_index=True)
    np.testing.assert_array_equal(first[0], again[0])
    np.testing.assert_array_equal(first[1], again[1])
    np.testing.assert_array_equal(first[0], ref("small", 0.05)[0])


@pytest.mark.parametrize("name,param", [("small", 0), ("small", 1), ("small", 2), ("flat", 2), ("big", 0)])
def test_hpd_collect(engines, name, param):
    v, eng, _ = engines(name)
    x = v[:, param, :].ravel()
    y = np.sort(x)
    m = hpd_ref.hpd_count(0.05, x.size)
    lo, hi = y[m - 1], y[x.size - m]
    nb, na = eng.hpd_collect(param, lo, hi, m - 1)
    assert (nb, na) == ((x < lo).sum(), (x > hi).sum())
    below, above = eng.hpd_get_tails(nb, na)
    np.testing.assert_array_equal(np.sort(below), np.sort(x[x < lo]))
    np.testing.assert_array_equal(np.sort(above), np.sort(x[x > hi]))


def test_hpd_collect_never_writes_past_cap(engines):
    """A cap one below the true count is an error, and the buffers past cap keep what an earlier,
    larger collect left there."""
    v, eng, _ = engines("small")
    x = v[:, 0, :].ravel()
    y = np.sort(x)
    big = hpd_ref.hpd_count(0.3, x.size)
    nb0, na0 = eng.hpd_collect(0, y[big - 1], y[x.size - big], big - 1)
    assert nb0 == na0 == big - 1                         # continuous draws: no ties
    below0, above0 = eng.hpd_get_tails(nb0, na0)
    m = hpd_ref.hpd_count(0.05, x.size)
    cap = m - 2                                          # the true counts are m - 1
    with pytest.raises(RuntimeError, match="room for"):
        eng.hpd_collect(0, y[m - 1], y[x.size - m], cap)
    below1, above1 = eng.hpd_get_tails(nb0, na0)
    np.testing.assert_array_equal(below1[cap:], below0[cap:])
    np.testing.assert_array_equal(above1[cap:], above0[cap:])
    assert (below1[:cap] < y[m - 1]).all() and (above1[:cap] > y[x.size - m]).all()   # cap slots were filled
    with pytest.raises(RuntimeError, match="no tails"):  # and the failed collect left no tails
        eng.hpd_gap(m, x.size, y[m - 1], y[x.size - m])


def _padded_gap(below, above, m, lo, hi):
    a = np.concatenate([np.sort(below), np.full(m - below.size, lo)])
    b = np.concatenate([np.full(m - above.size, hi), np.sort(above)])
    i = int(np.argmin(b - a))
    return np.array([a[i], b[i]]), i


M_GAP = 6000
SIZES = (0, 1, 63, 64, 65, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1, M_GAP - 1)


@pytest.mark.parametrize("q", range(len(SIZES)))
def test_set_tails_then_gap(engines, q):
    """The device half of the sharded path on hand-made tails: sizes around the wavefront and the
    sort tile, 0 and m - 1, every size once as `below` and once as `above`; half the values rounded
    to a coarse grid, so there are ties within the tails and in b - a."""
    _, eng, _ = engines("small")
    nb, na = SIZES[q], SIZES[-1 - q]
    rng = np.random.default_rng(100 + q)
    lo, hi = -1.25, 2.5
    below = lo - np.abs(rng.normal(size=nb)) * np.ldexp(1.0, rng.integers(-40, 41, size=nb)) - 2.0 ** -30
    above = hi + np.abs(rng.normal(size=na)) * np.ldexp(1.0, rng.integers(-40, 41, size=na)) + 2.0 ** -30
    below[::2] = np.floor(below[::2] * 4.0) / 4.0 - 0.25
    above[::2] = np.ceil(above[::2] * 4.0) / 4.0 + 0.25
    assert (below < lo).all() and (above > hi).all()
    eng.hpd_set_tails(below, above)
    got, idx = eng.hpd_gap(M_GAP, 100000, lo, hi)
    want, widx = _padded_gap(below, above, M_GAP, lo, hi)
    np.testing.assert_array_equal(got, want)
    assert idx == widx
    sb, sa = eng.hpd_get_tails(nb, na)                   # sorted in place by the gap call
    np.testing.assert_array_equal(sb, np.sort(below))
    np.testing.assert_array_equal(sa, np.sort(above))


def test_gap_with_more_tiles_than_one_scan_chunk(engines):
    """More than 256 sort tiles: the offsets' scan carries from one chunk of tiles into the next.
    Integers below 2^40 times 2^U{-30..0}: every key byte but the top one varies, with ties."""
    _, eng, _ = engines("flat")
    nb = 256 * SORT_TILE + 777
    rng = np.random.default_rng(7)
    below = -1.0 - rng.integers(1, 1 << 40, size=nb).astype(np.float64) * np.ldexp(1.0, rng.integers(-30, 1, size=nb))
    above = np.array([3.0, 2.5, 2.5])
    lo, hi, m = -1.0, 2.0, nb + 9
    eng.hpd_set_tails(below, above)
    got, idx = eng.hpd_gap(m, 4 * m, lo, hi)
    want, widx = _padded_gap(below, above, m, lo, hi)
    np.testing.assert_array_equal(got, want)
    assert idx == widx
    np.testing.assert_array_equal(eng.hpd_get_tails(nb, 0)[0], np.sort(below))


def test_hpd_argument_checks(engines):
    _, eng, _ = engines("small")
    eng.hpd_set_tails(np.array([-3.0, -2.0]), np.array([5.0]))
    for args, msg in (((0, 10, -1.0, 1.0), "1 <= m <= total"), ((11, 10, -1.0, 1.0), "1 <= m <= total"),
                      ((2, 10, -1.0, 1.0), "more than m - 1"), ((3, 10, 1.0, -1.0), "do not overlap")):
        with pytest.raises(RuntimeError, match=msg):
            eng.hpd_gap(*args)
    got, idx = eng.hpd_gap(6, 10, 1.0, -1.0)             # 2 m > total: lo > hi is the overlapping case
    want, widx = _padded_gap(np.array([-3.0, -2.0]), np.array([5.0]), 6, 1.0, -1.0)
    np.testing.assert_array_equal(got, want)
    assert idx == widx
    with pytest.raises(RuntimeError, match="out of range"):
        eng.hpd_collect(3, 0.0, 1.0, 5)
    with pytest.raises(RuntimeError, match="exceed"):
        eng.hpd_get_tails(10_000_000, 0)                 # the engine of `small` never held that many


def test_hpd_of_sampler_output(mamba):
    m = mamba.line().setsamplers([mamba.AMWG(["beta", "s2"], 1.0)])
    K = 96
    sim = mamba.mcmc(m, mamba.model.LINE_DATA, mamba.model.line_init_matrix(K, seed=5), 260, burnin=60, thin=2,
                     chains=K, keep_device=True)
    assert sim.value.shape == (100, 3, K)
    for alpha in (0.05, 0.5):
        vals, _ = sim.hpd(alpha)
        np.testing.assert_array_equal(vals, hpd_ref.hpd(sim.value, alpha)[0])
