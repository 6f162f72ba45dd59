"""Env-steps/s of the synthetic-spec actor at the same M: the device
synthetic rollout (graph replay) against the CPU VectorSynthetic + torch-actor
loop, at the HalfCheetah spec (17, 6) and the Humanoid spec (376, 17).

The device figure covers everything an actor rank's episode does on the GPU
(reset, policy forwards, noise, mixing GEMM, ticks with the n-step emit, tree
rebuild); the CPU figure is the stepping loop with the VecNStep fold.  Each
figure is the median of --repeats timed passes, with min and max.  The
horizon is short so that a run stays in seconds; one JSON line per
(spec, M).

    python scripts/synth_rollout_bench.py [--envs 1024 8192] [--horizon 50]
"""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from d4pg_amd.envs.vector import VecNStep, VectorSynthetic    # noqa: E402
from d4pg_amd.models import actor, critic                     # noqa: E402

H, K = 256, 51
SPECS = [(17, 6, 1.0), (376, 17, 0.4)]


def device_rate(net, vec, n, repeats, episodes):
    from d4pg_amd.ops import FusedEngine
    o, a, m, horizon = vec.obs_dim, vec.act_dim, vec.n, vec.horizon
    dist = {"type": "categorical", "v_min": -10.0, "v_max": 1.0, "n_atoms": K}
    eng = FusedEngine(obs_dim=o, act_dim=a, hidden=H, n_atoms=K, batch=64,
                      capacity=m * horizon, v_min=-10.0, v_max=1.0,
                      gamma_n=0.99 ** n, tau=0.001, lr_actor=1e-4,
                      lr_critic=1e-4, seed=0)
    c = critic(o, a, dist, hidden=H)
    eng.load_from_modules(net, net, c, c)
    eng.synth_rollout_alloc(m, n, vec.W, vec.U, horizon=horizon,
                            act_high=float(vec.act_high), seed=1)
    eng.synth_rollout_run(2)                # capture + warm
    rates = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        steps, _ = eng.synth_rollout_run(episodes)      # synchronizes
        rates.append(steps / (time.perf_counter() - t0))
    return rates


def cpu_rate(net, vec, n, repeats):
    rng = np.random.default_rng(2)
    fold = VecNStep(vec.n, vec.obs_dim, vec.act_dim, n, 0.99)
    rates = []
    for rep in range(repeats + 1):          # first pass is the warm-up
        t0 = time.perf_counter()
        obs = vec.reset()
        fold.reset()
        rows = 0
        with torch.no_grad():
            for _ in range(vec.horizon):
                a = net(torch.from_numpy(obs)).numpy()
                a = np.clip(a + 0.3 * rng.standard_normal(a.shape), -1.0,
                            1.0).astype(np.float32)
                obs2, r, done = vec.step(a)
                out = fold.push(obs, a, r, obs2, done)
                rows += 0 if out is None else len(out[2])
                obs = obs2
        if rep:
            rates.append(vec.n * vec.horizon / (time.perf_counter() - t0))
    return rates


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--envs", type=int, nargs="+", default=[1024, 8192])
    p.add_argument("--horizon", type=int, default=50)
    p.add_argument("--n_steps", type=int, default=3)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--episodes", type=int, default=10)
    p.add_argument("--no_cpu", action="store_true")
    args = p.parse_args()
    for o, a, hi in SPECS:
        torch.manual_seed(0)
        net = actor(o, a, hidden=H)
        for m in args.envs:
            vec = VectorSynthetic(m, o, a, horizon=args.horizon, act_high=hi,
                                  seed=1)
            out = {"obs": o, "act": a, "envs": m, "horizon": args.horizon,
                   "n_steps": args.n_steps}
            dev = device_rate(net, vec, args.n_steps, args.repeats,
                              args.episodes)
            out.update(device_env_steps_per_s=statistics.median(dev),
                       device_min=min(dev), device_max=max(dev))
            if not args.no_cpu:
                cpu = cpu_rate(net, vec, args.n_steps, args.repeats)
                out.update(cpu_env_steps_per_s=statistics.median(cpu),
                           cpu_min=min(cpu), cpu_max=max(cpu))
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
