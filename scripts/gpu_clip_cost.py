#!/usr/bin/env python3
"""Steps/s of the fused train step with and without gradient clipping.

    python scripts/gpu_clip_cost.py [--batch B] [--hidden H] [--steps N]
           [--warmup W] [--clip C] [--tree DIR]

Times one train_steps(N) call after W warm-up steps (a single persistent
launch at B <= 256, graph replay above) and prints one JSON line.  --clip
1e30 keeps all of the clip-on work and never binds.  --tree DIR imports the
package from another checkout (a build of the parent commit, say), so both
sides of a comparison are timed by the same code; such a tree need not know
max_grad_norm as long as --clip is 0.
"""

import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--hidden", type=int, default=256)
ap.add_argument("--steps", type=int, default=4000)
ap.add_argument("--warmup", type=int, default=400)
ap.add_argument("--clip", type=float, default=0.0)
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))
opts = ap.parse_args()
sys.path.insert(0, os.path.abspath(opts.tree))

import torch  # noqa: E402
from d4pg_amd.models import actor, critic  # noqa: E402
from d4pg_amd.ops import FusedEngine  # noqa: E402

SPG = 32
kw = {"max_grad_norm": opts.clip} if opts.clip > 0 else {}
eng = FusedEngine(obs_dim=3, act_dim=1, hidden=opts.hidden, n_atoms=51,
                  batch=opts.batch, capacity=1000000, v_min=-300.0, v_max=0.0,
                  gamma_n=0.99 ** 5, tau=0.001, lr_actor=1e-4, lr_critic=1e-4,
                  seed=0, **kw)
torch.manual_seed(0)
dist = {"type": "categorical", "v_min": -300.0, "v_max": 0.0, "n_atoms": 51}
a = actor(3, 1, hidden=opts.hidden)
c = critic(3, 1, dist, hidden=opts.hidden)
eng.load_from_modules(a, a, c, c)
eng.synth_fill(1000000, seed=7)
eng.train_steps(max(opts.warmup // SPG, 1) * SPG, steps_per_graph=SPG)
n = (opts.steps // SPG) * SPG
t0 = time.perf_counter()
eng.train_steps(n, steps_per_graph=SPG)
dt = time.perf_counter() - t0
print(json.dumps({"tree": os.path.abspath(opts.tree), "batch": opts.batch,
                  "hidden": opts.hidden, "clip": opts.clip, "steps": n,
                  "steps_per_sec": round(n / dt, 1),
                  "us_per_step": round(1e6 * dt / n, 2)}), flush=True)
