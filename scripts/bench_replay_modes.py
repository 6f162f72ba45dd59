#!/usr/bin/env python3
"""Prioritized against uniform replay on one MI355X, same build, same run:
learner grad-steps/s at the flagship (B=64, H=256) and the wide (B=4096,
H=1024) config over a 1e6-row replay, and Pendulum rollout env-steps/s at
M=1024 (uniform replay drops the per-episode tree sweep).  One JSON line per
measurement; medians over --reps interleaved repetitions.
"""

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

DIST = {"type": "categorical", "v_min": -300.0, "v_max": 0.0, "n_atoms": 51}


def make_engine(obs, act, hidden, batch, cap, prioritized):
    from d4pg_amd.models import actor, critic
    from d4pg_amd.ops import FusedEngine
    eng = FusedEngine(obs_dim=obs, act_dim=act, hidden=hidden, n_atoms=51,
                      batch=batch, capacity=cap, v_min=-300.0, v_max=0.0,
                      gamma_n=0.99 ** 5, tau=0.001, lr_actor=1e-4,
                      lr_critic=1e-3, seed=0, prioritized=prioritized)
    torch.manual_seed(0)
    a = actor(obs, act, hidden=hidden)
    c = critic(obs, act, DIST, hidden=hidden)
    eng.load_from_modules(a, a, c, c)
    return eng


def bench_learner(name, obs, act, hidden, batch, cap, steps, reps):
    engs = {p: make_engine(obs, act, hidden, batch, cap, p)
            for p in (True, False)}
    for eng in engs.values():
        eng.synth_fill(cap, seed=7)
        eng.train_steps(max(200, steps // 10))
    rates = {True: [], False: []}
    for _ in range(reps):
        for p, eng in engs.items():
            t0 = time.perf_counter()
            eng.train_steps(steps)
            rates[p].append(steps / (time.perf_counter() - t0))
    for p in (True, False):
        print(json.dumps({
            "config": name, "replay": "per" if p else "uniform",
            "grad_steps_per_sec": statistics.median(rates[p]),
            "min": min(rates[p]), "max": max(rates[p]), "batch": batch,
            "hidden": hidden, "capacity": cap, "reps": reps}), flush=True)


def bench_rollout(m, cap, episodes, reps):
    engs = {p: make_engine(3, 1, 256, 64, cap, p) for p in (True, False)}
    for eng in engs.values():
        eng.rollout_alloc(m, 5, horizon=200, seed=3)
        eng.rollout_run(2)
    rates = {True: [], False: []}
    for _ in range(reps):
        for p, eng in engs.items():
            t0 = time.perf_counter()
            env_steps, _ = eng.rollout_run(episodes)
            rates[p].append(env_steps / (time.perf_counter() - t0))
    for p in (True, False):
        print(json.dumps({
            "config": "pendulum_rollout", "replay": "per" if p else "uniform",
            "env_steps_per_sec": statistics.median(rates[p]),
            "min": min(rates[p]), "max": max(rates[p]), "n_envs": m,
            "capacity": cap, "reps": reps}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20000)
    args = ap.parse_args()
    bench_learner("flagship_b64_h256", 3, 1, 256, 64, 1_000_000, args.steps,
                  args.reps)
    bench_learner("wide_b4096_h1024", 17, 6, 1024, 4096, 1_000_000,
                  max(200, args.steps // 40), args.reps)
    bench_rollout(1024, 1_000_000, 5, args.reps)


if __name__ == "__main__":
    main()
