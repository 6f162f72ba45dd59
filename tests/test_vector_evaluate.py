"""vector_evaluate (d4pg_amd/envs/vector.py), the host twin of the device
evaluation, against M scalar greedy episodes (her.rollout_episode with
noise=False) from the same start states.

Tolerances are the twin-vs-scalar reward bounds of test_vector_env.py
(rtol 1e-5, atol 1e-6 per step) and test_vector_synth.py (1e-5 per step),
summed over the horizon.  Goal returns are integers and, with no distance
within 1e-3 of `tol` (asserted on the scalar envs), exact.
"""

import numpy as np
import pytest
import torch

from d4pg_amd.envs import NormalizeAction
from d4pg_amd.envs.goal_reach import GoalReachEnv
from d4pg_amd.envs.pendulum import PendulumEnv
from d4pg_amd.envs.synthetic import SyntheticEnv
from d4pg_amd.envs.vector import (VectorGoalReach, VectorPendulum,
                                  VectorSynthetic, vector_evaluate)
from d4pg_amd.her import rollout_episode

M = 5


def _net(o, a, gain=60.0, seed=4):
    from d4pg_amd.models import actor
    torch.manual_seed(seed)
    net = actor(o, a, hidden=64)
    with torch.no_grad():
        net.fc3.weight.mul_(gain)       # spread the actions over (-1, 1)
    return net


class _Greedy:
    """The scalar policy surface rollout_episode drives."""

    def __init__(self, net):
        self.net = net

    def select_action(self, obs, explore=True):
        assert not explore
        with torch.no_grad():
            a = self.net(torch.as_tensor(obs, dtype=torch.float32)
                         .reshape(1, -1)).numpy().reshape(-1)
        return np.clip(a, -1.0, 1.0)


class _StartAt:
    """A scalar env whose reset() lands on a given state."""

    def __init__(self, env, place):
        self.env_, self.place = env, place

    def __getattr__(self, name):
        return getattr(self.env_, name)

    def reset(self):
        self.env_.reset()
        return self.place(getattr(self.env_, "wrapped", self.env_))

    def step(self, a):
        return self.env_.step(a)


class _ZeroRng:
    def standard_normal(self, size):
        return np.zeros(size)


def _check_summary(summary, arrays, episodes=1):
    ret, length, succ = arrays
    assert ret.dtype == np.float64 and ret.shape == (M,)
    assert summary["mean_return"] == np.sum(ret, dtype=np.float64) / M
    assert summary["min_return"] == ret.min()
    assert summary["max_return"] == ret.max()
    assert summary["success_rate"] == succ.sum() / M
    assert summary["env_steps"] == int(length.sum())
    assert summary["episodes"] == episodes


def test_pendulum_matches_scalar_episodes():
    hor = 10
    net = _net(3, 1)
    rng = np.random.default_rng(1)
    th0 = rng.uniform(-np.pi, np.pi, M)
    td0 = rng.uniform(-1.0, 1.0, M)
    vec = VectorPendulum(M, seed=0, horizon=hor)
    vec.th, vec.thdot, vec.t = th0.copy(), td0.copy(), 0
    summary, arrays = vector_evaluate(net, vec, reset=False)
    want = []
    for i in range(M):
        def place(e, i=i):
            e.th, e.thdot = th0[i], td0[i]
            return e._obs()
        env = NormalizeAction(PendulumEnv(seed=0))
        env._max_episode_steps = hor
        ep, R, ok = rollout_episode(_Greedy(net), _StartAt(env, place),
                                    noise=False)
        assert len(ep) == hor and not ok
        want.append(R)
    ret, length, succ = arrays
    print("pendulum max abs err", np.abs(ret - want).max())
    np.testing.assert_allclose(ret, want, rtol=1e-5, atol=hor * 1e-6)
    assert (length == hor).all() and (succ == 0).all()
    assert np.ptp(ret) > 1.0            # the envs differ
    _check_summary(summary, arrays)


def test_goal_matches_scalar_episodes():
    hor, d, speed, tol = 12, 2, 0.1, 0.3
    net = _net(2 * d, d, gain=200.0)
    rng = np.random.default_rng(2)
    # search starts until the greedy episodes include a success and a
    # run to the horizon, none within the margin of tol
    for _ in range(200):
        pos0 = rng.uniform(-0.6, 0.6, (M, d)).astype(np.float32)
        goal0 = np.clip(pos0 + rng.uniform(-0.7, 0.7, (M, d)), -1.0,
                        1.0).astype(np.float32)
        want, margins = [], []
        for i in range(M):
            def place(e, i=i):
                e.pos = pos0[i].astype(np.float64)
                e.goal = goal0[i].astype(np.float64)
                return e._dict_obs()
            env = GoalReachEnv(dim=d, speed=speed, tol=tol, seed=0)
            env._max_episode_steps = hor
            ep, R, ok = rollout_episode(_Greedy(net), _StartAt(env, place),
                                        noise=False)
            want.append((R, len(ep), ok))
            margins += [abs(np.linalg.norm(
                np.asarray(s[3]["achieved_goal"], np.float64)
                - goal0[i]) - tol) for s in ep]
        oks = [w[2] for w in want]
        if min(margins) > 1e-3 and any(oks) and not all(oks):
            break
    else:
        pytest.fail("no start set with a success, a failure and the margin")
    vec = VectorGoalReach(M, dim=d, speed=speed, tol=tol, horizon=hor)
    vec.set_state(pos0, goal0)
    summary, arrays = vector_evaluate(net, vec, reset=False)
    ret, length, succ = arrays
    assert np.array_equal(ret, [w[0] for w in want])
    assert np.array_equal(length, [w[1] for w in want])
    assert np.array_equal(succ, [int(w[2]) for w in want])
    _check_summary(summary, arrays)


def test_synthetic_matches_scalar_episodes():
    o, a, hor, act_high = 5, 3, 8, 0.7
    net = _net(o, a)
    state0 = (0.5 * np.random.default_rng(3).standard_normal((M, o))
              ).clip(-1, 1).astype(np.float32)
    vec = VectorSynthetic(M, o, a, horizon=hor, act_high=act_high, seed=5,
                          proc_sigma=0.0)
    vec.set_state(state0)
    summary, arrays = vector_evaluate(net, vec, reset=False)
    want = []
    for i in range(M):
        def place(e, i=i):
            e.state = state0[i].astype(np.float64)
            e.rng = _ZeroRng()
            return e.state.astype(np.float32).copy()
        env = NormalizeAction(SyntheticEnv(o, a, horizon=hor,
                                           act_high=act_high, seed=5))
        ep, R, _ = rollout_episode(_Greedy(net), _StartAt(env, place),
                                   noise=False, max_steps=hor)
        assert len(ep) == hor
        want.append(R)
    ret, length, succ = arrays
    print("synthetic max abs err", np.abs(ret - want).max())
    np.testing.assert_allclose(ret, want, rtol=0, atol=hor * 1e-5)
    assert (length == hor).all() and (succ == 0).all()
    _check_summary(summary, arrays)


def test_episodes_accumulate_and_reset():
    vec = VectorPendulum(M, seed=3, horizon=4)
    net = _net(3, 1)
    summary, arrays = vector_evaluate(net, vec, episodes=3)
    assert summary["episodes"] == 3 and summary["env_steps"] == 3 * M * 4
    assert summary["min_return"] <= arrays[0].min()
    assert summary["max_return"] >= arrays[0].max()
    # an agent holding the module as .actor is accepted too
    class Agent:
        actor = net
    vec2 = VectorPendulum(M, seed=3, horizon=4)
    assert vector_evaluate(Agent(), vec2, episodes=3)[0] == summary


def test_unknown_vector_env_is_refused():
    class Other:
        n, horizon = 2, 3
    with pytest.raises(TypeError, match="unsupported vector env"):
        vector_evaluate(_net(3, 1), Other())
    with pytest.raises(ValueError):
        vector_evaluate(_net(3, 1), VectorPendulum(2), episodes=0)
