"""--async_collect 1 through the product path: after a serial warmup every
Worker cycle opens a collection window on the learner's own engine, trains
inside it, commits it and evaluates."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M, HOR, N = 64, 8, 3


def test_async_closed_loop_pendulum(tmp_path):
    from d4pg_amd.algo.d4pg import DDPG
    from d4pg_amd.config import (configure_env_params, critic_dist_info,
                                 make_parser)
    from d4pg_amd.envs import make, obs_act_dims
    from d4pg_amd.parallel.worker import Worker

    args = make_parser().parse_args(
        ["--env", "Pendulum-v1", "--vector_envs", str(M), "--max_steps",
         str(HOR), "--n_steps", str(N), "--warmup", "64",
         "--episodes_per_cycle", "64", "--train_steps_per_cycle", "8",
         "--eval_trials", "16", "--rmsize", "20000", "--bsize", "64",
         "--n_eps", "1", "--cycles_per_epoch", "3", "--debug", "0",
         "--seed", "0", "--async_collect", "1"])
    configure_env_params(args)
    env = make(args.env, seed=0)
    env._max_episode_steps = args.max_steps
    obs_dim, act_dim = obs_act_dims(env, her=False)
    agent = DDPG(obs_dim, act_dim, env=env, memory_size=args.rmsize,
                 batch_size=args.bsize, gamma=args.gamma, tau=args.tau,
                 prioritized_replay=True,
                 critic_dist_info=critic_dist_info(args),
                 n_steps=args.n_steps, device="cuda", backend="hip", seed=0)
    w = Worker("t", args, agent, env, run_dir=str(tmp_path))
    assert w.device_kind() == "pendulum"

    def step(action):
        raise AssertionError("env.step called on the device path")
    env.step = step
    evals = []
    real_eval = w.evaluate

    def evaluate():
        evals.append(real_eval())
        return evals[-1]
    w.evaluate = evaluate
    w.work(max_cycles=3)
    eng = agent.engine.engine
    assert eng.info()["collect_max_episodes"] == 1
    assert not eng.collect_pending()
    cnt = eng.counters()
    assert cnt["adam_t_actor"] == 24 == agent.train_steps_done
    # the warmup's rows plus three windows' rows
    rows = M * (HOR - N + 1)
    assert cnt["size"] == 4 * rows == w.device_rows
    assert w.env_meter.count == 4 * M * HOR
    assert len(evals) == 3
    assert all(np.isfinite(m) and 0.0 <= s <= 1.0 for m, s in evals)
