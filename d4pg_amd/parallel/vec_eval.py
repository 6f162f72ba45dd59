"""What the vector / device collect and evaluate paths of the Worker and of
the distributed ranks share: which of the three modelled env kinds a made
env is, the rollout producer that models it, and the greedy evaluator over
``eval_trials`` vector envs (FusedEngine.evaluate on a GPU, vector_evaluate on
the CPU twin).
"""

from __future__ import annotations

import numpy as np


def env_kind(args, env):
    """'pendulum' / 'goal' / 'synth' when ``env`` is one of the kinds the
    device rollouts and their host twins model, else None: Pendulum;
    GoalReach with --her 1; an env that unwraps to a SyntheticEnv (the test
    is on the instance, not the id — a gym install would resolve the same id
    to a real simulator)."""
    from ..envs.synthetic import SyntheticEnv
    base = getattr(env, "wrapped", env)
    name = str(getattr(args, "env", ""))
    if not args.her and name.startswith("Pendulum"):
        return "pendulum"
    if args.her and name.startswith("GoalReach"):
        return "goal"
    if not args.her and isinstance(base, SyntheticEnv):
        return "synth"
    return None


def producer_rows(kind, m, horizon, n_steps):
    """Replay rows one device episode of M envs can write at most."""
    real = m * max(1, horizon - n_steps + 1)
    return real + m * horizon if kind == "goal" else real


def alloc_producer(eng, kind, args, env, m, seed):
    """Allocate the rollout producer of ``kind`` with M envs on ``eng`` from
    the run's flags and the made env's parameters; returns the bound run
    method (its result starts (env_steps, rows, ...))."""
    horizon = int(env._max_episode_steps)
    noise = dict(noise=getattr(args, "noise", "gaussian"),
                 eps=float(getattr(args, "noise_eps", 0.3)),
                 ou_theta=args.ou_theta, ou_sigma=args.ou_sigma,
                 ou_mu=args.ou_mu, seed=int(seed))
    if kind == "pendulum":
        eng.rollout_alloc(m, args.n_steps, horizon=horizon, gamma=args.gamma,
                          **noise)
        return eng.rollout_run
    if kind == "goal":
        eng.goal_rollout_alloc(
            m, args.n_steps, horizon=horizon, gamma=args.gamma,
            speed=env.speed, tol=env.tol,
            her_ratio=float(getattr(args, "her_ratio", 0.8)), **noise)
        return eng.goal_rollout_run
    base = getattr(env, "wrapped", env)
    eng.synth_rollout_alloc(
        m, args.n_steps, np.asarray(base.W, np.float32),
        np.asarray(base.U, np.float32), horizon=horizon, gamma=args.gamma,
        act_high=float(base.action_space.high[0]),
        proc_sigma=float(base.proc_sigma), **noise)
    return eng.synth_rollout_run


def make_twin(kind, env, m, seed):
    """The host vector twin of ``env`` with M envs."""
    from ..envs.vector import (VectorGoalReach, VectorPendulum,
                               VectorSynthetic)
    horizon = int(env._max_episode_steps)
    if kind == "pendulum":
        return VectorPendulum(m, seed=seed, horizon=horizon)
    if kind == "goal":
        return VectorGoalReach(m, dim=env.dim, speed=env.speed, tol=env.tol,
                               seed=seed, horizon=horizon)
    base = getattr(env, "wrapped", env)
    vec = VectorSynthetic(
        m, base.obs_dim, base.act_dim, horizon=horizon,
        act_high=float(base.action_space.high[0]),
        seed=None, proc_sigma=base.proc_sigma,
        noise_seed=seed)
    # the twin must simulate THIS env, whatever seed named it
    vec.W = np.asarray(base.W, np.float32)
    vec.U = np.asarray(base.U, np.float32)
    return vec


class VectorEvaluator:
    """Greedy evaluation of a broadcast actor over ``eval_trials`` vector envs
    of ``env``'s kind.  With ``use_gpu`` an engine of its own, built like the
    actor ranks', with the producer that models the env and the device
    evaluation allocated on it; the actor is loaded with load_slab before each
    evaluation.  Otherwise vector_evaluate over the host twin."""

    def __init__(self, args, env, kind, obs_dim, act_dim, seed, use_gpu,
                 hidden=256):
        self.kind, self.trials = kind, int(args.eval_trials)
        self.engine = self.twin = None
        if use_gpu:
            from ..ops import FusedEngine
            horizon = int(env._max_episode_steps)
            self.engine = FusedEngine(
                obs_dim=obs_dim, act_dim=act_dim, hidden=hidden,
                n_atoms=args.n_atoms, batch=64,
                capacity=producer_rows(kind, self.trials, horizon,
                                       args.n_steps),
                v_min=args.v_min, v_max=args.v_max,
                gamma_n=args.gamma ** args.n_steps, tau=args.tau,
                lr_actor=1e-4, lr_critic=1e-4, seed=seed + 31)
            alloc_producer(self.engine, kind, args, env, self.trials,
                           seed + 37)
            self.engine.eval_alloc(self.trials, horizon=horizon)
        else:
            self.twin = make_twin(kind, env, self.trials, seed + 17)

    def evaluate(self, actor):
        """(mean_return, success_rate) of one evaluation episode."""
        if self.engine is not None:
            from ..ops import pack_net
            self.engine.load_slab("actor", pack_net(actor))
            r = self.engine.evaluate(1)
        else:
            from ..envs.vector import vector_evaluate
            r, _ = vector_evaluate(actor, self.twin, 1)
        return float(r["mean_return"]), float(r["success_rate"])
