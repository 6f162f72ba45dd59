"""The closed on-GPU cycle through the product path: a Worker with
--vector_envs M on the hip backend collects, trains and evaluates on the
learner's own engine (device rollout -> on-HBM replay -> fused step -> device
evaluation) and never steps the host env."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M, HOR, N = 64, 20, 3


def _worker(tmp_path, env_id, extra=(), vector_envs=M):
    from d4pg_amd.algo.d4pg import DDPG
    from d4pg_amd.config import (configure_env_params, critic_dist_info,
                                 make_parser)
    from d4pg_amd.envs import make, obs_act_dims
    from d4pg_amd.parallel.worker import Worker

    args = make_parser().parse_args(
        ["--env", env_id, "--vector_envs", str(vector_envs),
         "--max_steps", str(HOR), "--n_steps", str(N), "--warmup", "64",
         "--episodes_per_cycle", "64", "--train_steps_per_cycle", "8",
         "--eval_trials", "16", "--rmsize", "20000", "--bsize", "64",
         "--n_eps", "1", "--cycles_per_epoch", "2", "--debug", "0",
         "--seed", "0", *extra])
    configure_env_params(args)
    env = make(args.env, seed=0)
    env._max_episode_steps = args.max_steps
    obs_dim, act_dim = obs_act_dims(env, her=bool(args.her))
    agent = DDPG(obs_dim, act_dim, env=env, memory_size=args.rmsize,
                 batch_size=args.bsize, gamma=args.gamma, tau=args.tau,
                 prioritized_replay=True,
                 critic_dist_info=critic_dist_info(args),
                 n_steps=args.n_steps, device="cuda", backend="hip", seed=0)
    w = Worker("t", args, agent, env, run_dir=str(tmp_path))
    return w, agent, env, args


def _forbid_step(env):
    def step(action):
        raise AssertionError("env.step called on the device path")
    env.step = step


def _run_closed(tmp_path, env_id, kind, extra=()):
    w, agent, env, args = _worker(tmp_path, env_id, extra)
    assert w.device_kind() == kind
    w.eval_fixed_starts = True
    _forbid_step(env)
    w.work(max_cycles=2)
    assert agent.train_steps_done == 16
    eng = agent.engine.engine
    cnt = eng.counters()
    assert cnt["adam_t_actor"] == 16
    # warm-up + two cycles, one device episode of M envs each
    assert cnt["size"] == min(w.device_rows, args.rmsize)
    assert w.env_meter.count > 0
    mean, succ = w.evaluate()
    assert np.isfinite(mean) and 0.0 <= succ <= 1.0
    # fixed starts: the engine's own evaluation repeats it exactly
    assert mean == eng.evaluate(1)["mean_return"]
    assert eng.eval_info()["E"] == 16
    return w, cnt


def test_closed_loop_pendulum(tmp_path):
    w, cnt = _run_closed(tmp_path, "Pendulum-v1", "pendulum")
    assert cnt["size"] == 3 * M * (HOR - N + 1)
    assert w.env_meter.count == 3 * M * HOR


def test_closed_loop_goal_her(tmp_path):
    w, cnt = _run_closed(tmp_path, "GoalReach-v0", "goal", ("--her", "1"))
    # at least the folded real rows of envs that ran past n steps, at most
    # real + one hindsight row per step
    assert 0 < w.device_rows <= 3 * (M * (HOR - N + 1) + M * HOR)


def test_closed_loop_synthetic(tmp_path):
    w, cnt = _run_closed(tmp_path, "Synthetic-5x3", "synth")
    assert cnt["size"] == 3 * M * (HOR - N + 1)


def test_scalar_path_is_intact(tmp_path):
    w, agent, env, args = _worker(tmp_path, "Pendulum-v1", vector_envs=0)
    assert w.device_kind() is None
    args.warmup = 1
    calls = []
    real = env.step

    def step(action):
        calls.append(1)
        return real(action)
    env.step = step
    w.warmup()
    assert len(calls) == HOR
    assert agent.engine is None         # nothing built before training
