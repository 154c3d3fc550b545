"""SliceSimplex throughput on the node-IR interpreter kernel (the specialised kernel declines such schemes).

  python tools/simplex_bench.py [--chains 16384] [--steps 200] [--warmup 50] [--reps 2] [--cases a,b]

Times, per case, one mmb_run window of `steps` iterations after a warm-up window: the engine's device
events around the window's launches (Engine.run(time_kernels=True), Engine.kernel_time) and the wall
time of the call ending in a sync.  Prints one JSON line per case and repeat.  Cases:

  eyes           doc/examples/eyes.jl as published (48 observations): [DGS(T), Slice([lambda0, theta]),
                 Slice(s2, transform), SliceSimplex(P, scale = 0.75)]
  eyes_p_fixed   the same model with the weight a constant, T ~ Categorical([0.6, 0.4]), and the scheme
                 without its last block: what ran before Dirichlet nodes could be sampled
  simplex32      tests/slicesimplex_ref.py model B: P ~ Dirichlet of 32 elements, T observed (40),
                 [SliceSimplex(P, scale = 0.5)]: the widest vertex matrix

eyes minus eyes_p_fixed is the cost of the new block.  bench.py stays the flagship's yardstick.
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
ap.add_argument("--cases", default="eyes,eyes_p_fixed,simplex32")
a = ap.parse_args()

import torch  # noqa: F401,E402
import _mamba_path  # noqa: E402

mb = _mamba_path.load()
ir = mb.ir
K = a.chains


def eyes():
    m = ir.eyes_model()
    m.setinputs(ir.eyes_inputs()).setsamplers(ir.eyes_scheme())
    two = ir.eyes_inits()
    return m, m.init_matrix([two[c % 2] for c in range(K)], K)


def eyes_p_fixed():
    m = ir.Model(
        y=ir.Stochastic(1, lambda lambda0, theta, T, s2: ir.Normal(lambda0 + theta * (T - 1), ir.sqrt(s2)), False),
        T=ir.Stochastic(1, lambda: ir.Categorical([0.6, 0.4]), False),
        lam=ir.Logical(1, lambda lambda0, theta, step: lambda0 + theta * step),
        lambda0=ir.Stochastic(lambda: ir.Normal(0.0, 1000.0), False),
        theta=ir.Stochastic(lambda: ir.Uniform(0.0, 1000.0), False),
        s2=ir.Stochastic(lambda: ir.InverseGamma(0.001, 0.001)))
    m.setinputs({"step": [0.0, 1.0]})
    m.setsamplers([mb.DGS("T"), mb.Slice(["lambda0", "theta"], [5.0, 1.0]), mb.Slice("s2", 2.0, transform=True)])
    two = [{k: v for k, v in d.items() if k != "P"} for d in ir.eyes_inits()]
    return m, m.init_matrix([two[c % 2] for c in range(K)], K)


def simplex32():
    import slicesimplex_ref as ref
    m, inputs, inits = ref.modelB(ir)
    m.setinputs(inputs).setsamplers([mb.SliceSimplex("P", scale=ref.MB_SCALE)])
    return m, m.init_matrix(inits(K), K)


CASES = {"eyes": eyes, "eyes_p_fixed": eyes_p_fixed, "simplex32": simplex32}

for name in a.cases.split(","):
    m, V = CASES[name]()
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
        print(json.dumps({"case": name, "rep": rep, "chains": K, "steps": a.steps, "kernel": eng.ir_jit()[1],
                          "device_ms": round(kms, 3), "wall_ms": round(dt * 1e3, 3), "launches": launches,
                          "chain_updates_per_s": K * a.steps / (kms * 1e-3) if kms > 0 else None,
                          "chain_updates_per_s_wall": K * a.steps / dt}), flush=True)
    eng.close()
