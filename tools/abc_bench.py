"""ABC throughput at the bench size (16384 chains) on doc/examples/line_abc.jl's scheme, and the published run.

  python tools/abc_bench.py [--chains 16384] [--steps 100] [--warmup 20] [--reps 2] [--maxdraw 100] [--nsim 3]
  python tools/abc_bench.py --published [--chains 256]

Times one mmb_run window of `steps` iterations after a warm-up window: the engine's device events around the
window's launches (Engine.run(time_kernels=True), Engine.kernel_time) and the wall time of the call ending in a
sync.  Prints one JSON line per repeat.  A chain-update is one sweep of the scheme's two ABC blocks, each of up to
maxdraw candidates with nsim simulated data sets.  --published runs line_abc once as published (10000 iterations,
burn-in 1000) and prints the pooled means of s2, beta[1] and beta[2].  bench.py stays the flagship's yardstick.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--chains", type=int, default=16384)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--maxdraw", type=int, default=100)
ap.add_argument("--nsim", type=int, default=3)
ap.add_argument("--published", action="store_true")
a = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: F401,E402
import _mamba_path  # noqa: E402

mb = _mamba_path.load()
ir = mb.ir
K = a.chains

if a.published:
    m = ir.line_abc_model().setsamplers(ir.line_abc_scheme())
    t0 = time.perf_counter()
    sim = mb.mcmc(m, ir.line_abc_inputs(), ir.line_abc_inits(K, seed=1), 10000, burnin=1000, chains=K, seed=20261021)
    dt = time.perf_counter() - t0
    v = sim.value
    print(json.dumps({"case": "line_abc_published", "chains": K, "iters": 10000, "burnin": 1000, "wall_s": round(dt, 2),
                      "pooled_mean": {n: float(v[:, i, :].mean()) for i, n in enumerate(sim.names)},
                      "pooled_median": {n: float(np.median(v[:, i, :])) for i, n in enumerate(sim.names)},
                      "acceptance": {b: round(s["rate"], 4) for b, s in sim.engine.accept_stats().items()}}), flush=True)
    sim.engine.close()
    sys.exit(0)

m = ir.line_abc_model().setinputs(ir.line_abc_inputs()).setsamplers(ir.line_abc_scheme(a.maxdraw, a.nsim))
V = m.init_matrix(ir.line_abc_inits(K, seed=1), K)
eng = mb.Engine(m)
for rep in range(a.reps):
    eng.init_chains(V, seed=20261021)
    eng.run(a.warmup, draws=False, time_kernels=True)
    eng.sync()
    t0 = time.perf_counter()
    eng.run(a.steps, burnin=a.warmup, draws=False, time_kernels=True)
    eng.sync()
    dt = time.perf_counter() - t0
    kms, launches, _ = eng.kernel_time()
    print(json.dumps({"case": "line_abc", "rep": rep, "chains": K, "steps": a.steps, "maxdraw": a.maxdraw, "nsim": a.nsim,
                      "kernel": eng.ir_jit()[1].split(" (")[0], "device_ms": round(kms, 3),
                      "wall_ms": round(dt * 1e3, 3), "launches": launches,
                      "chain_updates_per_s": K * a.steps / (kms * 1e-3) if kms > 0 else None,
                      "chain_updates_per_s_wall": K * a.steps / dt,
                      "acceptance": {b: round(v["rate"], 4) for b, v in eng.accept_stats().items()}}), flush=True)
eng.close()
