"""The optimistic factorization pass's split square root and seeded reciprocal (samplers.h
pchol32_impl, device.h mmb_sqrt_prefix / mmb_sqrt_finish / mmb_rcp_seeded) against the oracle's
dpstf2 (oracle.c orc_pchol: C sqrt and division), through mmb_debug_pchol and through the AMM
update.

The matrices are near-diagonal: off-diagonals of 2^-40 sqrt(S_ii S_kk), so every squared factor
entry is below 2^-79 of its row's diagonal and rounds away in diag - work.  The successive pivot
candidates are then the diagonal values themselves, in descending order, while every row update
lij = (S_ip - dot) * (1 / ajj) shows the last bit of the pivot's root and reciprocal.  The
diagonals descend by three binades per step (distinct high words: no tie), with one crafted value
at the first, a middle or the last step:

* 4^k (1 - n 2^-53), n = 1..16 -- n = 1, 2 are the roots with an all-ones significand, where the
  seeded reciprocal's final correction may round wrongly;
* 2^k (1 +- n 2^-52), n = 0..16, k odd and even;
* 2^700, 2^-700 and values just inside them;
* values 65..80 ulps off a power of two: the first ones outside mmb_rcp_seeded_doubt, which the
  short sequence itself must get right;
* ordinary values.

plus dense SPD and indefinite matrices.  Expected redo flags are computed on the host from the
oracle's factor: the candidates of every step (diag - work, work summed as the kernel sums it),
then the post-loop check's conditions -- a high-word tie at the maximum, a pivot outside
[2^-700, 2^700], a zero candidate at the stop, and the new predicate.  The flag is per wavefront
(two chains), so clean cases are paired with clean ones and must come back without a redo: their
bits are the optimistic pass's own."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CH = 8  # chains per mmb_debug_pchol call: one workgroup


def doubt(x):
    """device.h mmb_rcp_seeded_doubt"""
    u = int(np.float64(x).view(np.uint64))
    return ((u + 64) & 0xFFFFFFFFFFFFF) <= 128


def ulps(x, n):
    return float((np.float64(x).view(np.int64) + np.int64(n)).view(np.float64))


def hiword(x):
    return int(np.float64(x).view(np.int64) >> 32)


def near_diagonal(diag_by_step, rng):
    """Matrix whose pivots are diag_by_step in that order, on shuffled elements."""
    d = len(diag_by_step)
    perm = rng.permutation(d)
    dg = np.empty(d)
    dg[perm] = diag_by_step
    r = np.sqrt(dg)
    U = rng.uniform(0.5, 1.0, (d, d)) * rng.choice([-1.0, 1.0], (d, d))
    S = np.tril(U, -1) * 2.0 ** -40 * np.outer(r, r)
    S = S + S.T
    np.fill_diagonal(S, dg)
    return S


def special_values(e, rng):
    """(label, value) with binary exponent e or e + 1 (or just below)."""
    ev = e if e % 2 == 0 else e + 1  # an even exponent: a power of four
    out = [("pow4_minus_%d" % n, 2.0 ** ev * (1.0 - n * 2.0 ** -53)) for n in range(1, 17)]
    for k in (e, e + 1):
        par = "even" if k % 2 == 0 else "odd"
        out += [("pow2%s_plus_%d" % (par, n), 2.0 ** k * (1.0 + n * 2.0 ** -52)) for n in range(0, 17)]
        out += [("pow2%s_minus_%d" % (par, n), 2.0 ** k * (1.0 - n * 2.0 ** -52)) for n in range(1, 17)]
    out += [("edge_plus_%d" % n, ulps(2.0 ** ev, n)) for n in range(65, 81, 3)]
    out += [("edge_minus_%d" % n, ulps(2.0 ** ev, -n)) for n in range(65, 81, 3)]
    out += [("ordinary_%d" % i, 2.0 ** e * rng.uniform(1.0, 2.0)) for i in range(2)]
    return out


def cases_for(d, rng):
    out = []
    E0 = 60
    base = lambda: [2.0 ** (E0 - 3 * i) * rng.uniform(1.0, 2.0) for i in range(d)]  # noqa: E731
    for t in sorted({0, d // 2, d - 1}):
        for label, v in special_values(E0 - 3 * t, rng):
            dg = base()
            dg[t] = v
            out.append(("%s@%d" % (label, t), near_diagonal(dg, rng)))
    # the bounds of the fast range: 2^700-ish first, 2^-700-ish last
    top = [("p700", 2.0 ** 700), ("p700_minus_1", ulps(2.0 ** 700, -1)), ("p700_inside", 2.0 ** 700 * (1 - 2.0 ** -30)),
           ("p700_outside", ulps(2.0 ** 700, 1))]
    bot = [("m700", 2.0 ** -700), ("m700_plus_1", ulps(2.0 ** -700, 1)), ("m700_inside", 2.0 ** -700 * (1 + 2.0 ** -30)),
           ("m700_outside", ulps(2.0 ** -700, -1))]
    for (lt, vt), (lb, vb) in zip(top, bot):
        for which in ("top", "bottom", "both"):
            dg = [2.0 ** (690 - 3 * i) * rng.uniform(1.0, 2.0) for i in range(d)]
            if which != "bottom":
                dg[0] = vt
            if which != "top":
                dg[d - 1] = vb
            out.append(("%s_%s_%s" % (lt, lb, which), near_diagonal(dg, rng)))
    for i in range(6):
        A = rng.normal(0.0, 1.0, (d, d + 3))
        out.append(("dense_spd_%d" % i, (A @ A.T) / d))
    for i in range(2):
        A = rng.normal(0.0, 1.0, (d, d + 3))
        S = (A @ A.T) / d
        S[i % d, i % d] = -1.0  # its candidate stays negative: the factorization stops before it
        out.append(("indefinite_%d" % i, S))
    return out


def redo_reasons(S, rank, L, piv):
    """The optimistic pass's post-loop check, from the oracle's factor: which of its conditions
    hold for this matrix (empty: the pass is not redone on its account)."""
    d = S.shape[0]
    reasons = set()
    work = np.zeros(d)
    remaining = list(range(d))
    for j in range(d):
        cand = {i: S[i, i] - work[i] for i in remaining}
        hw = {i: hiword(c) for i, c in cand.items()}
        mx = max(hw.values())
        if j == rank:  # dpstf2 stopped here: every candidate is <= 0; +0.0 has a non-negative key
            if mx >= 0:
                reasons.add("zero_at_stop")
            break
        if sum(1 for i in remaining if hw[i] == mx) > 1:
            reasons.add("tie")
        p = int(piv[j])
        assert cand[p] == max(cand.values())
        if not (2.0 ** -700 <= cand[p] <= 2.0 ** 700):
            reasons.add("range")
        elif doubt(cand[p]):
            reasons.add("doubt")
        remaining.remove(p)
        for i in remaining:
            lij = np.float64(L[i, j])
            work[i] = work[i] + lij * lij
    return reasons


@pytest.mark.parametrize("d", [2, 3, 17, 30])
def test_crafted_pivots_match_dpstf2(mamba, oracle, d):
    rng = np.random.default_rng(4100 + d)
    cases = cases_for(d, rng)
    ref = []
    for label, M in cases:
        ro, Lo, po = oracle.pchol(M)
        Lo = Lo.reshape(d, d)
        ref.append((ro, Lo, po, redo_reasons(M, ro, Lo, po)))
    # clean cases first, so that they share wavefronts with clean cases (one odd one out at most)
    order = sorted(range(len(cases)), key=lambda c: bool(ref[c][3]))
    clean_waves = doubt_only_waves = 0
    for lo in range(0, len(order), CH):
        idx = order[lo:lo + CH]
        rank, redone, L, piv = mamba.abi.debug_pchol(np.stack([cases[c][1] for c in idx]))
        for k, c in enumerate(idx):
            label = cases[c][0]
            ro, Lo, po, why = ref[c]
            assert rank[k] == ro, (label, rank[k], ro)
            if ro == d:
                np.testing.assert_array_equal(piv[k], po, err_msg=label)
                np.testing.assert_array_equal(L[k], Lo, err_msg=label)
            wave = [idx[q] for q in (k, k ^ 1) if q < len(idx)]
            wave_why = set().union(*(ref[q][3] for q in wave))
            assert redone[k] == (1 if wave_why else 0), (label, d, redone[k], wave_why)
            if k % 2 == 0:
                clean_waves += not wave_why
                doubt_only_waves += wave_why == {"doubt"}
    assert clean_waves >= 8, clean_waves            # the optimistic pass's own bits were compared
    assert doubt_only_waves >= 8, doubt_only_waves  # redone on account of the predicate alone
    by_label = {cases[c][0]: ref[c][3] for c in range(len(cases))}
    assert by_label["pow4_minus_1@0"] == {"doubt"} and by_label["pow4_minus_2@%d" % (d - 1)] == {"doubt"}
    assert not by_label["edge_plus_65@0"] and not by_label["edge_minus_65@%d" % (d // 2)]
    assert not by_label["p700_inside_m700_inside_both"] and by_label["p700_outside_m700_outside_top"] == {"range"}
    assert all(r[0] < d for (l, _), r in zip(cases, ref) if l.startswith("indefinite"))
    assert all(r[0] == d for (l, _), r in zip(cases, ref) if l.startswith("dense_spd"))


def _amm_slices(mamba, m):
    out, off = [], 0
    for s in m.samplers:
        d = m.block_dim(s)
        if s.kind == mamba.abi.MMB_SAMPLER_AMM:
            out.append((off, d))
            off += 4 + 2 * d + d * (d + 1)
        elif s.kind == mamba.abi.MMB_SAMPLER_AMWG:
            off += 2 + 2 * d
    return out


def test_amm_update_with_written_moments_matches_oracle(mamba, oracle):
    """Rats Gibbs+AMM, 64 chains x 12 iterations from tune rows written with mmb_set_tune: m = 2^20,
    Mv = 0 and a near-diagonal Mvv whose diagonal descends through distinct high words, so every
    update factorizes at full rank and every proposal after the first is the carried one, formed
    from the factor rows (Lrow[j] = the new root) still in registers.  Values, draws and every tune
    field equal the oracle's."""
    m = mamba.rats()
    m.setinputs(mamba.model.RATS_DATA)
    m.setsamplers(mamba.model.rats_scheme_gibbs_amm())
    K = 64
    init = mamba.model.rats_init_ls(K, seed=17)
    rng = np.random.default_rng(23)
    eng = mamba.Engine(m)
    eng.init_chains(init, seed=77)
    st = oracle.new_state(m, init)
    tune = eng.tune()
    tri = lambda i: i * (i + 1) // 2  # noqa: E731
    for c in range(K):
        for (off, d), scale in zip(_amm_slices(mamba, m), (1.0, 0.01)):
            T = d * (d + 1) // 2
            t = tune[c, off:off + 4 + 2 * d + 2 * T]
            t[:] = 0.0
            t[0], t[1] = 1.0, float(2 ** 20)
            dg = scale * 2.0 ** (-(c % 4)) * (1.0 + rng.permutation(d) / 64.0)
            Mvv = t[4 + d:4 + d + T]
            for i in range(d):
                for k in range(i):
                    Mvv[tri(i) + k] = 2.0 ** -10 * rng.uniform(-1.0, 1.0) * np.sqrt(dg[i] * dg[k])
                Mvv[tri(i) + i] = dg[i]
    eng.set_tune(tune)
    st["tune"][:, :st["tl"]] = tune
    oracle.amm_stats(reset=True)
    dg_ = eng.run(12, burnin=0, thin=1)
    do = oracle.run(m, st, 12, burnin=0, thin=1, seed=77, nthreads=8)
    np.testing.assert_array_equal(dg_, do)
    np.testing.assert_array_equal(eng.values(), st["values"])
    np.testing.assert_array_equal(eng.tune(), st["tune"][:, :st["tl"]])
    sg, so = eng.amm_stats(), oracle.amm_stats(reset=True)
    for b in sg:
        assert (sg[b]["updates"], sg[b]["full_rank"], sg[b]["rank_sum"]) == \
            (so[b]["updates"], so[b]["full_rank"], so[b]["rank_sum"]), (b, sg[b], so[b])
        assert sg[b]["full_rank"] > sg[b]["updates"] // 2, sg[b]
    eng.close()
