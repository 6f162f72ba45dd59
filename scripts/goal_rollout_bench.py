"""Env-steps/s of the goal-reaching HER actor at the same M: the device goal
rollout (graph replay) against the CPU VectorGoalReach path.

env steps are the real ones, sum of the per-env episode lengths.  The
device figure covers everything an actor rank's episode does on the GPU
(reset, policy forwards, ticks, count/scan/emit, tree rebuild); the CPU
figure is given for the stepping loop alone and with vector_add_experience.

    python scripts/goal_rollout_bench.py [--envs 8192] [--horizon 50]
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

from d4pg_amd.envs.vector import VectorGoalReach          # noqa: E402
from d4pg_amd.her import vector_add_experience            # noqa: E402
from d4pg_amd.models import actor, critic                 # noqa: E402

D, H, K = 2, 256, 51


class _Sink:
    def __init__(self):
        self.n = 0

    def add(self, *row):
        self.n += 1


def device_rate(net, m, n, horizon, repeats, episodes):
    from d4pg_amd.ops import FusedEngine
    dist = {"type": "categorical", "v_min": -50.0, "v_max": 0.0, "n_atoms": K}
    eng = FusedEngine(obs_dim=2 * D, act_dim=D, hidden=H, n_atoms=K, batch=64,
                      capacity=2 * m * horizon, v_min=-50.0, v_max=0.0,
                      gamma_n=0.99 ** n, tau=0.001, lr_actor=1e-4,
                      lr_critic=1e-4, seed=0)
    c = critic(2 * D, D, dist, hidden=H)
    eng.load_from_modules(net, net, c, c)
    eng.goal_rollout_alloc(m, n, horizon=horizon, seed=1)
    eng.goal_rollout_run(2)                 # capture + warm
    rates, rows, succ = [], 0, 0
    for _ in range(repeats):
        t0 = time.perf_counter()
        steps, rows, succ = eng.goal_rollout_run(episodes)   # synchronizes
        rates.append(steps / (time.perf_counter() - t0))
    return rates, rows / episodes, succ / (episodes * m)


def cpu_rate(net, m, n, horizon, repeats):
    vec = VectorGoalReach(m, dim=D, seed=1, horizon=horizon)
    rng = np.random.default_rng(2)
    step_rates, full_rates = [], []
    for rep in range(repeats + 1):          # first pass is the warm-up
        t0 = time.perf_counter()
        obs = vec.reset()
        alive = vec.alive
        with torch.no_grad():
            for _ in range(horizon):
                if not alive.any():
                    break
                a = net(torch.from_numpy(obs)).numpy()
                a = a + 0.3 * rng.standard_normal(a.shape)
                obs, _, _, alive = vec.step(a.astype(np.float32))
        t1 = time.perf_counter()
        ep_pos, ep_act, length, succ, goal = vec.episode()
        vector_add_experience(_Sink(), vec, ep_pos, ep_act, length, succ,
                              goal, her_ratio=0.8, n_steps=n, rng=rng)
        t2 = time.perf_counter()
        if rep:
            step_rates.append(length.sum() / (t1 - t0))
            full_rates.append(length.sum() / (t2 - t0))
    return step_rates, full_rates


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--envs", type=int, default=8192)
    p.add_argument("--horizon", type=int, default=50)
    p.add_argument("--n_steps", type=int, default=3)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--episodes", type=int, default=20)
    p.add_argument("--cpu_repeats", type=int, default=2)
    a = p.parse_args()
    torch.manual_seed(0)
    net = actor(2 * D, D, hidden=H)
    out = {"envs": a.envs, "horizon": a.horizon, "n_steps": a.n_steps}
    dev, rows, succ = device_rate(net, a.envs, a.n_steps, a.horizon,
                                  a.repeats, a.episodes)
    out.update(device_env_steps_per_s=statistics.median(dev),
               device_min=min(dev), device_max=max(dev),
               rows_per_episode=rows, success_fraction=succ)
    step, full = cpu_rate(net, a.envs, a.n_steps, a.horizon, a.cpu_repeats)
    out.update(cpu_step_loop_env_steps_per_s=statistics.median(step),
               cpu_with_relabel_env_steps_per_s=statistics.median(full))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
