#!/usr/bin/env python3
"""The categorical (C51) against the quantile critic head on one MI355X, same
build, same run: learner grad-steps/s at the flagship (B=64, H=256, K=51) and
the wide (B=4096, H=1024, K=51) config over a 1e6-row replay.  The two
engines' repetitions are interleaved; one JSON line per head with the median
and the min-max of --reps repetitions.  --gemm_precision bf16 measures the
wide config with bf16 MFMA operands (both heads).
"""

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

K = 51
DISTS = {
    "categorical": {"type": "categorical", "v_min": -300.0, "v_max": 0.0,
                    "n_atoms": K},
    "quantile": {"type": "quantile", "n_atoms": K, "kappa": 1.0},
}


def make_engine(obs, act, hidden, batch, cap, dist, gemm_precision):
    from d4pg_amd.models import actor, critic
    from d4pg_amd.ops import FusedEngine
    eng = FusedEngine(obs_dim=obs, act_dim=act, hidden=hidden, n_atoms=K,
                      batch=batch, capacity=cap, v_min=-300.0, v_max=0.0,
                      gamma_n=0.99 ** 5, tau=0.001, lr_actor=1e-4,
                      lr_critic=1e-3, seed=0, dist=dist, kappa=1.0,
                      gemm_precision=gemm_precision if batch > 512 else "fp32")
    torch.manual_seed(0)
    a = actor(obs, act, hidden=hidden)
    c = critic(obs, act, DISTS[dist], hidden=hidden)
    eng.load_from_modules(a, a, c, c)
    return eng


def bench_learner(name, obs, act, hidden, batch, cap, steps, reps,
                  gemm_precision):
    engs = {d: make_engine(obs, act, hidden, batch, cap, d, gemm_precision)
            for d in DISTS}
    for eng in engs.values():
        eng.synth_fill(cap, seed=7)
        eng.train_steps(max(200, steps // 10))
    rates = {d: [] for d in DISTS}
    for _ in range(reps):
        for d, eng in engs.items():
            t0 = time.perf_counter()
            eng.train_steps(steps)
            rates[d].append(steps / (time.perf_counter() - t0))
    for d, eng in engs.items():
        cnt = eng.counters()
        print(json.dumps({
            "config": name, "dist": d,
            "grad_steps_per_sec": statistics.median(rates[d]),
            "min": min(rates[d]), "max": max(rates[d]), "batch": batch,
            "hidden": hidden, "n_atoms": K, "capacity": cap, "reps": reps,
            "gemm_precision": eng.gemm_precision,
            "persistent": bool(eng.info()["persistent"]),
            "loss_critic": cnt["loss_critic"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--gemm_precision", default="fp32",
                    choices=["fp32", "bf16"])
    args = ap.parse_args()
    bench_learner("flagship_b64_h256", 3, 1, 256, 64, 1_000_000, args.steps,
                  args.reps, args.gemm_precision)
    bench_learner("wide_b4096_h1024", 17, 6, 1024, 4096, 1_000_000,
                  max(200, args.steps // 40), args.reps, args.gemm_precision)


if __name__ == "__main__":
    main()
