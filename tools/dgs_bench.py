"""DGS throughput on the node-IR interpreter kernel (the specialised kernel declines DGS schemes).

  python tools/dgs_bench.py [--chains 16384] [--steps 200] [--warmup 50] [--reps 2]

Times, per case, one mmb_run window of `steps` iterations after a warm-up window: the engine's device
events around the window's launches (Engine.run(time_kernels=True), Engine.kernel_time) and the wall
time of the call ending in a sync.  Prints one JSON line per case and repeat.  The models are the
test models of tests/dgs_ref.py:

  mixture_data   T ~ Categorical (40 elements, 3 values), y ~ Normal(mu[T], s), mu data: [DGS(T)]
  mixture_rwm    the same with mu sampled: [DGS(T), RWM(mu)]

One DGS update of T evaluates 40 elements x 3 candidates x (own term + the 40-element y node).
bench.py stays the flagship's yardstick.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--chains", type=int, default=16384)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=50)
ap.add_argument("--reps", type=int, default=2)
a = ap.parse_args()

import torch  # noqa: F401,E402
import _mamba_path  # noqa: E402
import dgs_ref  # noqa: E402

mb = _mamba_path.load()
K = a.chains


def case(make, scheme):
    m, inputs, inits = make(mb.ir)
    m.setinputs(inputs).setsamplers(scheme)
    return m, m.init_matrix(inits(K), K)


CASES = {"mixture_data": lambda: case(dgs_ref.model2, [mb.DGS("T")]),
         "mixture_rwm": lambda: case(dgs_ref.model3, [mb.DGS("T"), mb.RWM("mu", 0.3)])}

for name, make in CASES.items():
    m, V = make()
    eng = mb.Engine(m)
    for rep in range(a.reps):
        eng.init_chains(V, seed=20261020)
        eng.run(a.warmup, draws=False, time_kernels=True)
        eng.sync()
        t0 = time.perf_counter()
        eng.run(a.steps, burnin=a.warmup, draws=False, time_kernels=True)
        eng.sync()
        dt = time.perf_counter() - t0
        kms, launches, _ = eng.kernel_time()
        print(json.dumps({"case": name, "rep": rep, "chains": K, "steps": a.steps, "kernel": eng.ir_jit()[1],
                          "device_ms": round(kms, 3), "wall_ms": round(dt * 1e3, 3), "launches": launches,
                          "chain_updates_per_s": K * a.steps / (kms * 1e-3) if kms > 0 else None,
                          "element_updates_per_s": K * a.steps * dgs_ref.M2_N / (kms * 1e-3) if kms > 0 else None,
                          "chain_updates_per_s_wall": K * a.steps / dt}), flush=True)
    eng.close()
