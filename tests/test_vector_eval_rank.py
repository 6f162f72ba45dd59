"""The distributed evaluator rank with --vector_envs > 0: eval_trials greedy
vector envs per round (vector_evaluate over the host twin on the CPU, the
device evaluation on a GPU) feeding the same EWMA, with the scalar host env
never stepped; with --vector_envs 0 the scalar episode as before."""

import numpy as np
import pytest
import torch

from d4pg_amd.config import configure_env_params, make_parser

KINDS = [("Pendulum-v1", (), "pendulum"),
         ("GoalReach-v0", ("--her", "1"), "goal"),
         ("Synthetic-5x3", (), "synth")]


def _node(env_id, extra=(), vector_envs=8, device="cpu"):
    from d4pg_amd.parallel.learner import DistributedD4PG
    args = make_parser().parse_args(
        ["--env", env_id, "--max_steps", "12", "--warmup", "0",
         "--rmsize", "2000", "--bsize", "32", "--n_steps", "3",
         "--debug", "0", "--eval_trials", "6", "--seed", "3",
         "--vector_envs", str(vector_envs), *extra])
    configure_env_params(args)
    # no process group: the node is built and its collect phase driven alone
    node = DistributedD4PG(args, rank=2, world=3, device=device)
    assert node.is_evaluator
    return node


def _count_steps(node):
    calls = []
    real = node.env.step

    def step(action):
        calls.append(1)
        return real(action)
    node.env.step = step
    return calls


@pytest.mark.parametrize("env_id,extra,kind", KINDS)
def test_evaluator_rank_uses_the_vector_twin(env_id, extra, kind):
    from d4pg_amd.envs.vector import vector_evaluate
    from d4pg_amd.parallel.vec_eval import make_twin
    # --gpu_actors 0: the twin path, also where a GPU is present
    node = _node(env_id, (*extra, "--gpu_actors", "0"))
    ve = node.vec_eval
    assert ve is not None and ve.kind == kind
    assert ve.engine is None and ve.twin.n == 6 and ve.twin.horizon == 12
    calls = _count_steps(node)
    # the same twin from the same seed gives the return the rank logs
    seed = 3 + 7919 * 2
    want, _ = vector_evaluate(node.agent.actor,
                              make_twin(kind, node.env, 6, seed + 17), 1)
    assert len(node._collect().items) == 0
    assert not calls
    assert node.ewma == want["mean_return"] and np.isfinite(node.ewma)
    first = node.ewma
    node._collect()
    assert node.ewma != first           # the EWMA moves with a new episode


def test_synthetic_twin_simulates_the_made_env():
    node = _node("Synthetic-5x3", ("--gpu_actors", "0"))
    base = node.env.wrapped
    twin = node.vec_eval.twin
    assert np.array_equal(twin.W, base.W.astype(np.float32))
    assert np.array_equal(twin.U, base.U.astype(np.float32))
    assert float(twin.proc_sigma) == np.float32(base.proc_sigma)
    assert float(twin.act_high) == float(base.action_space.high[0])


def test_scalar_evaluator_rank_is_unchanged():
    node = _node("Pendulum-v1", vector_envs=0)
    assert node.vec_eval is None
    calls = _count_steps(node)
    node._collect()
    assert len(calls) == 12 and np.isfinite(node.ewma)


@pytest.mark.gpu
@pytest.mark.parametrize("env_id,extra,kind", KINDS)
def test_evaluator_rank_uses_the_device_evaluation(env_id, extra, kind):
    from d4pg_amd.ops import pack_net
    node = _node(env_id, extra)
    ve = node.vec_eval
    assert ve is not None and ve.twin is None and ve.engine is not None
    info = ve.engine.eval_info()
    assert (info["E"], info["horizon"]) == (6, 12)
    calls = _count_steps(node)
    node._collect()
    assert not calls and np.isfinite(node.ewma)
    # the broadcast actor was loaded into the engine's slab
    assert torch.equal(ve.engine.store_slab("actor"),
                       pack_net(node.agent.actor))
    res = ve.engine.eval_results()
    assert node.ewma == res["sum"] / res["count"] and res["count"] == 6


@pytest.mark.gpu
def test_gpu_actors_zero_keeps_the_evaluator_on_the_twin():
    node = _node("Pendulum-v1", ("--gpu_actors", "0"))
    assert node.vec_eval.engine is None and node.vec_eval.twin is not None


def test_worker_refuses_a_replay_below_one_device_episode():
    """The device path names the flags to change before any engine exists."""
    from d4pg_amd.envs import make
    from d4pg_amd.parallel.worker import Worker
    args = make_parser().parse_args(
        ["--env", "GoalReach-v0", "--her", "1", "--vector_envs", "64",
         "--max_steps", "20", "--n_steps", "3", "--warmup", "1",
         "--rmsize", "2000", "--seed", "0"])
    configure_env_params(args)
    env = make(args.env, seed=0)
    env._max_episode_steps = args.max_steps

    class Agent:
        backend, memory_size = "hip", 2000

        def ensure_engine(self):
            raise AssertionError("engine built before the capacity check")
    w = Worker("t", args, Agent(), env)
    assert w.device_kind() == "goal"
    # 64 * (20 - 3 + 1) real + 64 * 20 hindsight rows = 2432 > 2000
    with pytest.raises(ValueError, match="--rmsize 2000 is below the 2432"):
        w.warmup()
