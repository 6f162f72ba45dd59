"""Greedy env-steps/s of the device evaluation next to the training rollout
of the same producer, on one engine and with one call pattern: E = M envs,
graph replay, the median of --repeats timed calls of --episodes episodes
(min and max alongside).  Pendulum at horizon 200 and the (17, 6) synthetic
spec at horizon 50; one JSON line each.

An evaluation tick does strictly less than a rollout tick (no rings, no emit,
no tree sweep), so a rate below the rollout's is a defect to explain.

    python scripts/eval_bench.py [--envs 8192] [--repeats 5] [--episodes 10]
"""

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from d4pg_amd.envs.vector import VectorSynthetic              # noqa: E402
from d4pg_amd.models import actor, critic                     # noqa: E402

H, K, N = 256, 51, 3


def _engine(o, a, capacity):
    from d4pg_amd.ops import FusedEngine
    dist = {"type": "categorical", "v_min": -10.0, "v_max": 1.0, "n_atoms": K}
    eng = FusedEngine(obs_dim=o, act_dim=a, hidden=H, n_atoms=K, batch=64,
                      capacity=capacity, v_min=-10.0, v_max=1.0,
                      gamma_n=0.99 ** N, tau=0.001, lr_actor=1e-4,
                      lr_critic=1e-4, seed=0)
    torch.manual_seed(0)
    net = actor(o, a, hidden=H)
    c = critic(o, a, dist, hidden=H)
    eng.load_from_modules(net, net, c, c)
    return eng


def _rates(run, steps_per_call, repeats):
    run()                                   # capture + warm
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        run()                               # synchronizes
        out.append(steps_per_call / (time.perf_counter() - t0))
    return out


def _line(name, m, horizon, eng, rollout_run, args):
    steps = m * horizon * args.episodes
    roll = _rates(lambda: rollout_run(args.episodes), steps, args.repeats)
    eng.eval_alloc(m, horizon=horizon)
    ev = _rates(lambda: eng.evaluate(args.episodes), steps, args.repeats)
    print(json.dumps({
        "env": name, "envs": m, "horizon": horizon,
        "eval_env_steps_per_s": statistics.median(ev),
        "eval_min": min(ev), "eval_max": max(ev),
        "rollout_env_steps_per_s": statistics.median(roll),
        "rollout_min": min(roll), "rollout_max": max(roll)}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--envs", type=int, default=8192)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--episodes", type=int, default=10)
    args = p.parse_args()
    m = args.envs

    eng = _engine(3, 1, m * 200)
    eng.rollout_alloc(m, N, horizon=200, seed=1)
    _line("Pendulum", m, 200, eng, eng.rollout_run, args)

    vec = VectorSynthetic(1, 17, 6, horizon=50, act_high=1.0, seed=1)
    eng = _engine(17, 6, m * 50)
    eng.synth_rollout_alloc(m, N, vec.W, vec.U, horizon=50, act_high=1.0,
                            seed=1)
    _line("Synthetic-17x6", m, 50, eng, eng.synth_rollout_run, args)


if __name__ == "__main__":
    main()
