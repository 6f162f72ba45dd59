"""Wall time per closed-loop cycle with and without overlapped collection
(--async_collect), on one GPU.

A cycle is what Worker.work runs on the device path: one collection of M
envs, `--train_steps` fused train steps, one greedy evaluation.  Serial:
rollout_run -> train_steps -> evaluate.  Async: collect_begin -> train_steps
-> collect_commit -> evaluate, the episodes on the rollout stream inside the
train launch.  Two configurations: Pendulum at M=1024, horizon 200, and the
synthetic 17/6 spec at M=8192, horizon 50; B=64, 600 train steps per cycle.
Each figure is over --repeats timed runs of --cycles cycles after --warm
cycles; min, median and max per cycle, profiler off.  --mode serial runs on
a build without the collect_* calls too, so the parent commit can be timed
with the same script.

Also reports the learner's grad-steps/s inside an open window against the
same engine with no window.

    python scripts/async_collect_bench.py [--mode serial async learner]
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

H, K, B = 256, 51, 64
CONFIGS = {
    # name: (obs, act, M, horizon, n)
    "pendulum_M1024": (3, 1, 1024, 200, 5),
    "synth17x6_M8192": (17, 6, 8192, 50, 3),
}


def build(name, window):
    from d4pg_amd.ops import FusedEngine
    o, a, m, hor, n = CONFIGS[name]
    rows = m * (hor - n + 1)
    dist = {"type": "categorical", "v_min": -300.0, "v_max": 0.0,
            "n_atoms": K}
    eng = FusedEngine(obs_dim=o, act_dim=a, hidden=H, n_atoms=K, batch=B,
                      capacity=8 * rows, v_min=-300.0, v_max=0.0,
                      gamma_n=0.99 ** n, tau=0.001, lr_actor=1e-4,
                      lr_critic=1e-4, seed=0)
    torch.manual_seed(0)
    net, c = actor(o, a, hidden=H), critic(o, a, dist, hidden=H)
    eng.load_from_modules(net, net, c, c)
    if name.startswith("pendulum"):
        eng.rollout_alloc(m, n, horizon=hor, seed=1)
        run = eng.rollout_run
    else:
        vec = VectorSynthetic(1, o, a, horizon=hor, act_high=1.0, seed=1)
        eng.synth_rollout_alloc(m, n, vec.W, vec.U, horizon=hor, seed=1)
        run = eng.synth_rollout_run
    eng.eval_alloc(16, horizon=hor)
    if window:
        eng.collect_alloc(1)
    run(1)                              # warmup fill, serial in both modes
    return eng, run


def cycle_times(name, mode, steps, cycles, warm, repeats):
    eng, run = build(name, mode == "async")

    def cycle():
        if mode == "async":
            eng.collect_begin(1)
            eng.train_steps(steps)
            eng.collect_commit()
        else:
            run(1)
            eng.train_steps(steps)
        eng.evaluate(1)

    for _ in range(warm):
        cycle()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(cycles):
            cycle()
        out.append((time.perf_counter() - t0) / cycles)
    return out


def learner_rates(name, steps, repeats):
    """grad-steps/s of train_steps(steps): no window, and inside a window
    whose episode is still running when the steps start."""
    eng, _ = build(name, True)
    eng.train_steps(steps)
    res = {"no_window": [], "in_window": []}
    for _ in range(repeats):
        t0 = time.perf_counter()
        eng.train_steps(steps)
        res["no_window"].append(steps / (time.perf_counter() - t0))
        eng.collect_begin(1)
        t0 = time.perf_counter()
        eng.train_steps(steps)
        res["in_window"].append(steps / (time.perf_counter() - t0))
        eng.collect_commit()
    return res


def stats(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--mode", nargs="+", default=["serial", "async", "learner"],
                   choices=["serial", "async", "learner"])
    p.add_argument("--configs", nargs="+", default=list(CONFIGS),
                   choices=list(CONFIGS))
    p.add_argument("--train_steps", type=int, default=600)
    p.add_argument("--cycles", type=int, default=20)
    p.add_argument("--warm", type=int, default=3)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--tag", default="")
    args = p.parse_args()
    for name in args.configs:
        for mode in args.mode:
            out = {"config": name, "mode": mode, "tag": args.tag,
                   "train_steps": args.train_steps}
            if mode == "learner":
                r = learner_rates(name, args.train_steps, args.repeats)
                out.update({k + "_grad_steps_per_s": stats(v)
                            for k, v in r.items()})
            else:
                ts = cycle_times(name, mode, args.train_steps, args.cycles,
                                 args.warm, args.repeats)
                out["cycle_ms"] = stats([1e3 * t for t in ts])
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
