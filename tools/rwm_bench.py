"""RWM throughput at the bench size (16384 chains), next to the same models under their AMWG / Slice
schemes as the reference point.

  python tools/rwm_bench.py [--chains 16384] [--steps 400] [--warmup 100] [--reps 2]

Times, per case, one mmb_run window of `steps` iterations after a warm-up window: the engine's device
events around the window's launches (Engine.run(time_kernels=True), Engine.kernel_time) and the wall
time of the call ending in a sync.  Prints one JSON line per case and repeat:

  dyes_ir_scheme4    dyes.jl:69-71 (RWM Cosine, RWM, Slice) via the node IR
  dyes_ir_reference  dyes.jl:58-59 (NUTS, Slice) via the node IR
  rats_rwm           pure RWM (five blocks, 30-element alpha / beta), hand-lowered
  rats_reference     rats.jl:112-116 (Slice, AMWG), hand-lowered
  rats_ir_rwm / rats_ir_reference   the same two via the node IR

MMB_IR_JIT=0 times the interpreter kernels.  bench.py stays the flagship's yardstick.
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
ap.add_argument("--steps", type=int, default=400)
ap.add_argument("--warmup", type=int, default=100)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--cases", default="")
a = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: F401,E402
import _mamba_path  # noqa: E402

mb = _mamba_path.load()
ir = mb.ir
K = a.chains


def rats_rwm():
    return [mb.RWM("s2_c", 0.3, mb.Cosine), mb.RWM("alpha", 1.0),
            mb.RWM(["mu_alpha", "s2_alpha"], [3.0, 0.5], mb.Triweight), mb.RWM("beta", 0.1, mb.SymUniform),
            mb.RWM(["mu_beta", "s2_beta"], [0.1, 0.5])]


def dyes(scheme):
    m = ir.dyes_model().setinputs(ir.dyes_inputs()).setsamplers(scheme)
    rng = np.random.default_rng(21)
    inits = [{"y": ir.DYES_Y, "theta": 1500.0, "s2_within": 1.0, "s2_between": 1.0,
              "mu": 1500.0 + rng.normal(0.0, 50.0, 6)} for _ in range(K)]
    return m, m.init_matrix(inits, K)


def rats(scheme):
    m = mb.rats().setinputs(mb.model.RATS_DATA).setsamplers(scheme)
    return m, mb.model.rats_init_ls(K)


def rats_ir(scheme):
    m = ir.rats_model().setinputs(ir.rats_inputs()).setsamplers(scheme)
    return m, m.init_matrix(ir.rats_inits_ls(K), K)


CASES = {
    "dyes_ir_scheme4": lambda: dyes([mb.RWM("theta", 50.0, mb.Cosine), mb.RWM("mu", 50.0),
                                     mb.Slice(["s2_within", "s2_between"], 1000.0)]),
    "dyes_ir_reference": lambda: dyes([mb.NUTS(["mu", "theta"]), mb.Slice(["s2_within", "s2_between"], 1000.0)]),
    "rats_rwm": lambda: rats(rats_rwm()),
    "rats_reference": lambda: rats(mb.model.rats_scheme_reference()),
    "rats_ir_rwm": lambda: rats_ir(rats_rwm()),
    "rats_ir_reference": lambda: rats_ir(mb.model.rats_scheme_reference()),
}

for name in (a.cases.split(",") if a.cases else CASES):
    m, V = CASES[name]()
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
        out = {"case": name, "rep": rep, "chains": K, "steps": a.steps, "blocks": len(m.samplers),
               "kernel": eng.ir_jit()[1].split(" (")[0] if m.kind == mb.abi.MMB_MODEL_IR else "static",
               "device_ms": round(kms, 3), "wall_ms": round(dt * 1e3, 3), "launches": launches,
               "chain_updates_per_s": K * a.steps / (kms * 1e-3) if kms > 0 else None,
               "chain_updates_per_s_wall": K * a.steps / dt,
               "rwm_acceptance": {b: round(v["rate"], 4) for b, v in eng.rwm_stats().items()}}
        print(json.dumps(out), flush=True)
    eng.close()
