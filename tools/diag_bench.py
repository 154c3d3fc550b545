"""Timing of the per-chain diagnostics at the bench size (rats, 16384 chains, 2000 kept draws).

  python tools/diag_bench.py [--iters 2000]

Prints one JSON line: the bytes of one pass over the draws and the wall time (each ending in a
sync) of autocor, changerate, gewekediag("imse") and, in the same process as the yardstick,
summarystats; and for the IMSE windows of gewekediag the lag pairs the rule added against the
sweeps the block scheme took (DG_PAIRS = 8 pairs per sweep; a wavefront sweeps until its last
lane's rule has fired).  For heideldiag("imse") and rafterydiag(q=0.1, r=0.05, s=0.9) (at the
defaults Nmin = 3746 exceeds the 2000 kept draws and no kernel would run): the wall times, the
passes each kernel's algorithm makes over its window, and per wavefront the sweeps of the
Raftery-Lewis selection (fixed by the digit width) and of its thinning loop (a wavefront sweeps
until its last lane's bic is negative; the sweep at kthin reads every kthin-th row).
For hpd(alpha = 0.05): the wall time of Chains.hpd, of quantile beside it, the sizes of the tails the
device sorts, and the route a user had without it (download the draws, np.sort each param, the gap
on the host).
Run under `rocprofv3 --kernel-trace --stats` for per-kernel durations.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=2000)
ap.add_argument("--chains", type=int, default=16384)
ap.add_argument("--reps", type=int, default=5)
a = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: F401,E402
import _mamba_path  # noqa: E402

mb = _mamba_path.load()
DG_PAIRS = 8
m = mb.rats()
m.setinputs(mb.model.RATS_DATA)
m.setsamplers(mb.model.rats_scheme_gibbs_amm())
eng = mb.Engine(m)
eng.init_chains(mb.model.rats_init_ls(a.chains, seed=1), seed=2)
eng.run(a.iters, burnin=0, thin=1, draws=False, keep_device=True)
eng.sync()
n = eng.num_kept()
nbytes = n * eng.pmon * a.chains * 8


def timed(f):
    out = f()                                  # warm
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        out = f()
        eng.sync()
    return (time.perf_counter() - t0) / a.reps, out


t_ac, (ac, _) = timed(lambda: mb.autocor(eng))
t_cr, cr = timed(lambda: mb.changerate_sharded(eng))
t_gw, gw = timed(lambda: mb.gewekediag(eng, etype="imse"))
t_ss, ss = timed(lambda: mb.summarystats_sharded(eng))

# IMSE block scheme on the two Geweke windows: pairs examined per lane = init + added + the one
# that broke; a wavefront (64 adjacent chains of one param) takes its slowest lane's sweeps
imse = {}
for name, (i0, i1) in zip(("first", "last"), mb.geweke_windows(n)):
    terms = eng.chain_mcse(i0, i1, "imse")[:, :, mb.diag.F_TERMS]          # K x p
    mpairs = (i1 - i0 - 2) // 2
    examined = np.minimum(terms + 2, mpairs + 1)
    sweeps = np.ceil(examined / DG_PAIRS)
    pad = (-sweeps.shape[0]) % 64
    wave = np.pad(sweeps, ((0, pad), (0, 0))).reshape(-1, 64, sweeps.shape[1]).max(1)
    imse[name] = {"window": [i0, i1], "window_bytes": (i1 - i0) * eng.pmon * a.chains * 8,
                  "pairs_added_mean": float(terms.mean()), "pairs_added_max": int(terms.max()),
                  "sweeps_lane_mean": float(sweeps.mean()), "sweeps_wave_mean": float(wave.mean()),
                  "sweeps_wave_max": int(wave.max())}

t_hd, hd = timed(lambda: mb.heideldiag(eng, etype="imse"))
RQ, RR, RS = 0.1, 0.05, 0.9
t_rf, rf = timed(lambda: mb.rafterydiag(eng, RQ, RR, RS))


def per_wave(x):
    """max over each wavefront (64 adjacent chains of one param) of a K x p array"""
    pad = (-x.shape[0]) % 64
    return np.pad(x, ((0, pad), (0, 0))).reshape(-1, 64, x.shape[1]).max(1)


# Heidelberger-Welch: the second-half mcse, two sweeps from row 0 for every candidate window,
# then the mcse of each series' chosen window (IMSE block sweeps as above, windows of mixed length)
starts, i_final = mb.diag.heidel_starts(n)
chosen = hd[:, 0, :].T.astype(np.int64)                            # Burn-in = i + start - 2 = the 0-based start at start = 1
chosen = np.where(hd[:, 1, :].T > 0, chosen, starts[-1])           # not converged: the last window tested
terms = eng.chain_mcse_from(chosen, n, "imse")[:, :, mb.diag.F_TERMS]
examined = np.minimum(terms + 2, (n - chosen - 2) // 2 + 1)
hw = per_wave(np.ceil(examined / DG_PAIRS))
heidel = {"candidates": starts, "cvm_passes": 2, "cvm_bytes": 2 * (n - starts[0]) * eng.pmon * a.chains * 8,
          "not_converged": float((hd[:, 1, :] == 0).mean()), "chosen_start_mean": float(chosen.mean()),
          "chosen_window_bytes": int((n - chosen).sum()) * 8,
          "mcse_from_sweeps_wave_mean": float(hw.mean()), "mcse_from_sweeps_wave_max": int(hw.max()),
          "test_passed": float(np.nanmean(hd[:, 5, :]))}

# Raftery-Lewis: 64 / DG_RF_BITS selection sweeps (+ 1 for the upper order statistic when the
# quantile index is fractional), then thinning sweeps kthin = 1 .. the wavefront's largest
DG_RF_BITS = 4
rfc = eng.chain_raftery(RQ)
kthin = np.nan_to_num(rfc[:, :, 1], nan=float(n // 2))
kw = per_wave(kthin)
sel = 64 // DG_RF_BITS + int(1.0 + (n - 1) * RQ != np.floor(1.0 + (n - 1) * RQ))
harm = np.array([sum(1.0 / k for k in range(1, int(x) + 1)) for x in kw.ravel()])
raftery = {"q": RQ, "r": RR, "s": RS, "selection_sweeps": sel,
           "kthin_lane_mean": float(kthin.mean()), "kthin_lane_max": int(kthin.max()),
           "thinning_sweeps_wave_mean": float(kw.mean()), "thinning_sweeps_wave_max": int(kw.max()),
           "thinning_rows_wave_mean_passes": float(harm.mean()),
           "passes_wave_mean": float(sel + harm.mean()), "ran_out": int(np.isnan(rfc[:, :, 1]).sum()),
           "dependence_factor_median": float(np.nanmedian(rf[:, 4, :]))}

# hpd(alpha = 0.05): 8 select passes + 1 collect pass over each param's draws, then the sort of the
# two tails (2 x (m - 1) keys, the digit passes in which the keys differ) and the gap reduction;
# quantile (the same select, 10 ranks) beside it, and the route a user had before: download the
# draws, np.sort each param, the gap on the host (a baseline, not the code under test)
sim = mb.Chains(np.empty((n, eng.pmon, 0)), m.monitor_names, 1, 1, np.arange(1, a.chains + 1), m, eng)
t_hpd, (hp, _) = timed(lambda: sim.hpd(0.05))
t_q, _ = timed(lambda: mb.quantile_sharded(eng))
N = n * a.chains
m_hpd = mb.summary.hpd_count(0.05, N)
tails = []
for j in range(eng.pmon):
    lo_j, hi_j = (float(v) for v in mb.summary.order_stats(eng, j, [m_hpd - 1, N - m_hpd]))
    tails.append(list(eng.hpd_collect(j, lo_j, hi_j, m_hpd - 1)))
t0 = time.perf_counter()
val = eng.draws()
t_dl = time.perf_counter() - t0
host = np.empty((eng.pmon, 2))
for j in range(eng.pmon):
    y = np.sort(val[:, j, :].ravel())
    d = y[N - m_hpd:] - y[:m_hpd]
    i = int(np.argmin(d))
    host[j] = y[i], y[N - m_hpd + i]
t_host = time.perf_counter() - t0
del val
hpd = {"alpha": 0.05, "m": m_hpd, "param_bytes": nbytes // eng.pmon, "tail_counts": tails, "hpd_s": t_hpd,
       "quantile_s": t_q, "host_route_s": t_host, "host_download_s": t_dl, "host_sort_gap_s": t_host - t_dl,
       "equals_host_route": bool(np.array_equal(hp, host)), "hpd": hp.tolist()}

print(json.dumps({"draws_bytes": nbytes, "kept": n, "chains": a.chains, "hpd": hpd,
                  "autocor_s": t_ac, "changerate_s": t_cr, "gewekediag_imse_s": t_gw, "summarystats_s": t_ss,
                  "heideldiag_imse_s": t_hd, "rafterydiag_s": t_rf, "heidel": heidel, "raftery": raftery,
                  "imse_blocks": imse, "changerate": cr.tolist(),
                  "autocor_mean": np.nanmean(ac, axis=2).tolist(),
                  "geweke_abs_z_gt_2": float(np.nanmean(np.abs(gw[:, 0, :]) > 2.0)),
                  "summarystats": ss.tolist()}))
