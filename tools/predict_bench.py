"""Timing of posterior prediction on the device-kept draws at the bench size (16384 chains, 2000 kept
draws), next to tools/modelstats_bench.py and on its two models.

  python tools/predict_bench.py [--iters 2000] [--chains 16384] [--reps 5] [--out profiles/predict_bench.json]

For the hand-lowered line model (P = 5 predicted columns) and for the node-IR seeds model with its
random effects monitored (26 monitored columns, P = 21 Binomial elements), writes one JSON object with
the wall time (every call ends in a sync; minimum, median and maximum over --reps after a warm-up) of
  Engine.draws_predict_moments   the predict kernel over every draw plus the moments reduction, in chunks
  Engine.draws_deviance          ms_ir_kernel / ms_line_kernel on the same input: the comparison
  Engine.chain_summary           one pass of ss_chain_kernel over every monitored column: the yardstick
and the bytes each must move, computed from the shapes: predict reads the columns its nodes need and
writes n x P x K doubles, the moments pass reads them back.  Run under `rocprofv3 --kernel-trace
--stats` (a run of its own, --reps 1) for the per-kernel durations.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=2000)
ap.add_argument("--chains", type=int, default=16384)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_bench.json"))
a = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: F401,E402
import _mamba_path  # noqa: E402

mb = _mamba_path.load()
ir = mb.ir


def line():
    m = mb.line()
    m.setinputs(mb.model.LINE_DATA)
    m.setsamplers([mb.AMWG(["beta", "s2"], 1.0)])
    return m, mb.model.line_init_matrix(a.chains, seed=1)


def seeds():
    m = ir.Model(
        r=ir.Stochastic(1, lambda alpha0, alpha1, x1, alpha2, x2, alpha12, b, n:
                        ir.Binomial(n, ir.invlogit(alpha0 + alpha1 * x1 + alpha2 * x2 + alpha12 * x1 * x2 + b)), False),
        b=ir.Stochastic(1, lambda s2: ir.Normal(0, ir.sqrt(s2))),
        alpha0=ir.Stochastic(lambda: ir.Normal(0, 1000)),
        alpha1=ir.Stochastic(lambda: ir.Normal(0, 1000)),
        alpha2=ir.Stochastic(lambda: ir.Normal(0, 1000)),
        alpha12=ir.Stochastic(lambda: ir.Normal(0, 1000)),
        s2=ir.Stochastic(lambda: ir.InverseGamma(0.001, 0.001)))
    m.setinputs(ir.SEEDS)
    m.setsamplers([mb.AMM(["alpha0", "alpha1", "alpha2", "alpha12"], 0.01 * np.eye(4)), mb.AMWG("b", 0.01),
                   mb.AMWG("s2", 0.1)])
    return m, m.init_matrix([ir.seeds_inits()[k % 2] for k in range(a.chains)], a.chains)


def bench(name, make):
    m, init = make()
    eng = mb.Engine(m)
    eng.init_chains(init, seed=2)
    eng.run(a.iters, burnin=0, thin=1, draws=False, keep_device=True)
    eng.sync()
    n = eng.num_kept()

    def timed(f):
        f()                                    # warm: code objects, allocations
        eng.sync()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            f()
            eng.sync()
            ts.append(time.perf_counter() - t0)
        return {"min_s": min(ts), "median_s": statistics.median(ts), "max_s": max(ts)}

    keys = m.keys("output")
    ids = mb.modelstats.node_ids(m, keys)
    need = mb.modelstats.needed_nodes(m, keys)
    ncols = sum(len([c for c in m.monitor_names if c == k or c.startswith(k + "[")]) for k in need)
    P = eng.predict_width(ids)
    shift = np.zeros(P)
    col_bytes = n * a.chains * 8
    t_pr = timed(lambda: eng.draws_predict_moments(ids, 2, 1, 1, shift))
    t_dev = timed(lambda: eng.draws_deviance(ids, 0.0))
    t_cs = timed(lambda: eng.chain_summary(np.zeros(eng.pmon), n, 0))
    out = {"model": name, "kept": n, "chains": a.chains, "monitored_columns": eng.pmon, "columns_read": ncols,
           "predicted_columns": P, "variates": n * a.chains * P,
           "predict_bytes": {"read": ncols * col_bytes, "written": P * col_bytes, "moments_read": P * col_bytes},
           "draws_bytes": eng.pmon * col_bytes,
           "draws_predict_moments": t_pr, "draws_deviance": t_dev, "chain_summary": t_cs,
           "variates_per_s": n * a.chains * P / t_pr["median_s"],
           "predict_moved_GBps": (ncols + 2 * P) * col_bytes / t_pr["median_s"] / 1e9,
           "chain_summary_GBps": eng.pmon * col_bytes / t_cs["median_s"] / 1e9,
           "predict_over_chain_summary": t_pr["median_s"] / t_cs["median_s"],
           "predict_over_deviance": t_pr["median_s"] / t_dev["median_s"]}
    eng.close()
    return out


res = {"line": bench("line", line), "seeds_ir": bench("seeds_ir", seeds)}
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
