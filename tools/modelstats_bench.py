"""Timing of dic / logpdf on the device-kept draws at the bench size (16384 chains, 2000 kept draws).

  python tools/modelstats_bench.py [--iters 2000] [--chains 16384]

For the hand-lowered line model and for the node-IR seeds model with its random effects monitored
(26 monitored columns, 21 observed Binomial elements), prints one JSON line with: the bytes of the
draws the kernel reads, the wall time (each ending in a sync) of Engine.draws_deviance (the
log-density kernel over every draw plus the per-chain reduction), of Chains.dic (two summary passes,
the density at the means, the deviance pass), and in the same process the yardstick of the device
summaries: one Engine.chain_summary call (one pass of ss_chain_kernel over every monitored column)
and summarystats_sharded.  Run under `rocprofv3 --kernel-trace --stats` for per-kernel durations.
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
ap.add_argument("--reps", type=int, default=3)
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
        out = f()                              # warm
        eng.sync()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            out = f()
            eng.sync()
        return (time.perf_counter() - t0) / a.reps, out

    keys = m.keys("output")
    ids = mb.modelstats.node_ids(m, keys)
    need = mb.modelstats.needed_nodes(m, keys)
    ncols = sum(len([c for c in m.monitor_names if c == k or c.startswith(k + "[")]) for k in need)
    sim = mb.Chains(np.empty((n, eng.pmon, 0)), m.monitor_names, 1, 1, np.arange(1, a.chains + 1), m, eng)
    t_dev, _ = timed(lambda: eng.draws_deviance(ids, 0.0))
    t_dic, (dic, _, _) = timed(lambda: sim.dic())
    t_cs, _ = timed(lambda: eng.chain_summary(np.zeros(eng.pmon), n, 0))
    t_ss, _ = timed(lambda: mb.summarystats_sharded(eng))
    col_bytes = n * a.chains * 8
    out = {"model": name, "kept": n, "chains": a.chains, "monitored_columns": eng.pmon, "columns_read": ncols,
           "bytes_read": ncols * col_bytes, "draws_bytes": eng.pmon * col_bytes,
           "draws_deviance_s": t_dev, "draws_per_s": n * a.chains / t_dev, "read_GBps": ncols * col_bytes / t_dev / 1e9,
           "dic_s": t_dic, "chain_summary_s": t_cs, "chain_summary_GBps": eng.pmon * col_bytes / t_cs / 1e9,
           "summarystats_s": t_ss, "deviance_over_chain_summary": t_dev / t_cs, "dic_over_summarystats": t_dic / t_ss,
           "dic": dic.tolist()}
    if m.kind == mb.abi.MMB_MODEL_IR:
        out["sweep_kernel"] = eng.ir_jit()[1].splitlines()[0] if eng.ir_jit()[1] else ""
    eng.close()
    return out


print(json.dumps({"line": bench("line", line), "seeds_ir": bench("seeds_ir", seeds)}))
