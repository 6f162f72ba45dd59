"""Vectorized environments + batched n-step folding.

The reference steps one env per worker process with a B=1 policy forward
per step (main.py:142-152) — ~25-30k env-steps/s per actor on this host.
The MI355X-native actor instead simulates M envs per process in numpy
batch form and runs ONE [M, obs] policy forward per tick, so each actor
rank feeds the learner 10-30x more transitions for the same process count.

VecNStep reproduces NStepFolder's semantics (replay/nstep.py — emit
(s_{t-n+1}, a_{t-n+1}, sum gamma^k r, s_{t+1}, done) once the window is
full; reset on episode end without flushing) in array form.  All M
pendulums share the fixed 200-step horizon, so episodes stay synchronized
and the window reset is a single buffer clear.
"""

from __future__ import annotations

import numpy as np

from .pendulum import angle_normalize


class VectorPendulum:
    """M independent Pendulum-v1 instances in numpy arrays.  Actions are
    NORMALIZED to (-1, 1) (the NormalizeAction convention); the affine map
    to [-2, 2] torque happens inside."""

    obs_dim = 3
    act_dim = 1
    horizon = 200
    max_speed = 8.0
    max_torque = 2.0
    dt = 0.05
    g = 10.0
    m = 1.0
    l = 1.0

    def __init__(self, n_envs: int, seed: int | None = None,
                 horizon: int | None = None):
        self.n = int(n_envs)
        self.rng = np.random.default_rng(seed)
        if horizon is not None:
            self.horizon = int(horizon)
        self.th = np.zeros(self.n)
        self.thdot = np.zeros(self.n)
        self.t = 0

    def reset(self) -> np.ndarray:
        self.th = self.rng.uniform(-np.pi, np.pi, self.n)
        self.thdot = self.rng.uniform(-1.0, 1.0, self.n)
        self.t = 0
        return self._obs()

    def _obs(self) -> np.ndarray:
        return np.stack([np.cos(self.th), np.sin(self.th), self.thdot],
                        axis=1).astype(np.float32)

    def step(self, actions: np.ndarray):
        """actions [M, 1] in (-1, 1).  Returns (obs, rewards, done) where
        done is a scalar — the synchronized horizon flag.  Auto-resets
        AFTER the caller has read the terminal obs via the return value."""
        u = np.clip(actions[:, 0], -1.0, 1.0) * self.max_torque
        cost = (angle_normalize(self.th) ** 2 + 0.1 * self.thdot ** 2
                + 0.001 * u ** 2)
        newthdot = self.thdot + (3.0 * self.g / (2.0 * self.l)
                                 * np.sin(self.th)
                                 + 3.0 / (self.m * self.l ** 2) * u) * self.dt
        self.thdot = np.clip(newthdot, -self.max_speed, self.max_speed)
        self.th = self.th + self.thdot * self.dt
        self.t += 1
        return self._obs(), (-cost).astype(np.float32), self.t >= self.horizon


class VecNStep:
    """Array-form n-step folder for M synchronized envs."""

    def __init__(self, n_envs: int, obs_dim: int, act_dim: int,
                 n_steps: int, gamma: float):
        self.m = n_envs
        self.n = max(1, int(n_steps))
        self.gamma = float(gamma)
        self.obs_dim, self.act_dim = obs_dim, act_dim
        self.reset()

    def reset(self):
        self._s = np.zeros((self.n, self.m, self.obs_dim), np.float32)
        self._a = np.zeros((self.n, self.m, self.act_dim), np.float32)
        self._r = np.zeros((self.n, self.m), np.float32)
        self._len = 0
        self._head = 0

    def push(self, s, a, r, s2, done_flag: bool):
        """Feed one synchronized step for all M envs; returns a matured
        (S, A, R, S2, D) tuple of [M, ...] arrays or None."""
        i = (self._head + self._len) % self.n      # tail slot
        self._s[i] = s
        self._a[i] = a
        self._r[i] = r
        if self._len < self.n:
            self._len += 1
        else:
            self._head = (self._head + 1) % self.n
        if self._len < self.n:
            return None
        start = self._head                          # oldest entry
        R = np.zeros(self.m, np.float32)
        for k in range(self.n):
            R += (self.gamma ** k) * self._r[(start + k) % self.n]
        out = (self._s[start].copy(), self._a[start].copy(), R,
               np.asarray(s2, np.float32).copy(),
               np.full(self.m, float(done_flag), np.float32))
        if done_flag:
            self.reset()
        return out


class VectorGoalReach:
    """M independent GoalReachEnv instances in float32 numpy arrays: a point
    in [-1, 1]^dim moved by a velocity action, sparse reward, success within
    ``tol`` of the goal.  Unlike VectorPendulum, episodes end PER ENV (on
    success): an env that has succeeded stays put (``alive`` 0) until the
    next reset, so env i has its own length ``len[i] <= horizon``.

    Host twin of the device goal rollout (ops/hip/engine_goal.hip): same
    float32 state and the same update order — clip the action, move, clip
    the position, record, then test success — so it serves both as the CPU
    vector-actor path and as the parity oracle.  The whole episode is
    recorded (``ep_pos [horizon+1, M, dim]``, ``ep_act [horizon, M, dim]``)
    because the "future" HER relabel needs it (her.vector_add_experience).
    """

    def __init__(self, n_envs: int, dim: int = 2, speed: float = 0.1,
                 tol: float = 0.05, seed: int | None = None,
                 horizon: int = 50):
        self.n = int(n_envs)
        self.dim = int(dim)
        self.obs_dim, self.act_dim = 2 * self.dim, self.dim
        self.speed = np.float32(speed)
        self.tol = np.float32(tol)
        self.horizon = int(horizon)
        self.rng = np.random.default_rng(seed)
        self.set_state(np.zeros((self.n, self.dim), np.float32),
                       np.zeros((self.n, self.dim), np.float32))

    def compute_reward(self, achieved_goal, desired_goal, info=None):
        """GoalReachEnv.compute_reward (float64 distance)."""
        d = np.linalg.norm(np.asarray(achieved_goal, np.float64)
                           - np.asarray(desired_goal, np.float64), axis=-1)
        return np.where(d <= float(self.tol), 0.0, -1.0)

    def set_state(self, pos, goal) -> np.ndarray:
        """Start an episode from the given positions and goals.  No success
        check here, as in GoalReachEnv.reset."""
        self.pos = np.array(pos, np.float32).reshape(self.n, self.dim)
        self.goal = np.array(goal, np.float32).reshape(self.n, self.dim)
        self.alive = np.ones(self.n, bool)
        self.len = np.zeros(self.n, np.int32)
        self.succ = np.zeros(self.n, bool)
        self.t = 0
        self.ep_pos = np.zeros((self.horizon + 1, self.n, self.dim),
                               np.float32)
        self.ep_act = np.zeros((self.horizon, self.n, self.dim), np.float32)
        self.ep_pos[0] = self.pos
        return self._obs()

    def reset(self) -> np.ndarray:
        return self.set_state(
            self.rng.uniform(-1.0, 1.0, (self.n, self.dim)),
            self.rng.uniform(-1.0, 1.0, (self.n, self.dim)))

    def _obs(self) -> np.ndarray:
        return np.concatenate([self.pos, self.goal], axis=1)

    def distance(self) -> np.ndarray:
        """float32 ||pos - goal||, summed over dims in ascending order as
        the kernel does."""
        d2 = np.zeros(self.n, np.float32)
        for k in range(self.dim):
            d = self.pos[:, k] - self.goal[:, k]
            d2 = d2 + d * d
        return np.sqrt(d2)

    def step(self, actions: np.ndarray):
        """actions [M, dim].  Returns (obs, reward, success, alive): reward
        is 0 / -1 for the envs that moved (0 for those already finished),
        success the per-env flag so far, alive the mask AFTER this step."""
        if self.t >= self.horizon:
            raise RuntimeError("VectorGoalReach: step past the horizon")
        live = self.alive.copy()
        a = np.clip(np.asarray(actions, np.float32), -1.0, 1.0)
        self.ep_act[self.t][live] = a[live]
        new = np.clip(self.pos + self.speed * a, np.float32(-1.0),
                      np.float32(1.0)).astype(np.float32)
        self.pos[live] = new[live]
        self.t += 1
        self.ep_pos[self.t][live] = self.pos[live]
        self.len[live] = self.t
        hit = live & (self.distance() <= self.tol)
        self.succ |= hit
        self.alive &= ~hit
        reward = np.where(live & ~hit, -1.0, 0.0).astype(np.float32)
        return self._obs(), reward, self.succ.copy(), self.alive.copy()

    def episode(self):
        """(ep_pos, ep_act, len, succ, goal) of the episode so far."""
        return (self.ep_pos, self.ep_act, self.len.copy(), self.succ.copy(),
                self.goal.copy())


# seed-xor constant of the device process-noise stream (engine_synth.hip
# k_syn_tick)
SYNTH_PROC_STREAM = 0x51A7E


class GeneratorProcNoise:
    """Process-noise source of VectorSynthetic backed by a numpy
    Generator (the default)."""

    def __init__(self, rng: np.random.Generator):
        self.rng = rng

    def reset(self):
        pass

    def draw(self, tick: int, n_envs: int, obs_dim: int) -> np.ndarray:
        return self.rng.standard_normal((n_envs, obs_dim))


class PhiloxProcNoise:
    """Process-noise source drawing what the device synthetic rollout
    draws (the role PhiloxHerRng plays for HER): the standard normal of dim
    k of env i at `tick` of rollout episode `episode` is the Box-Muller of
    the first two philox words keyed by (seed ^ SYNTH_PROC_STREAM,
    (episode << 20) | (tick + 2), (k << 32) | i).  The uniforms are the
    kernel's float32 (0, 1] map; the transcendental part is float64.
    ``reset()`` moves on to the next episode, as the device epoch does."""

    def __init__(self, seed: int, episode: int = 0):
        self.seed, self.episode = int(seed), int(episode)

    def reset(self):
        self.episode += 1

    @staticmethod
    def _u01(x: int) -> np.float32:
        return np.float32(np.float32(np.float32(np.uint32(x))
                                     + np.float32(1.0))
                          * np.float32(2.3283064e-10))

    def normal(self, tick: int, env: int, dim: int) -> float:
        from ..her import philox4x32_10
        w = philox4x32_10(self.seed ^ SYNTH_PROC_STREAM,
                          (self.episode << 20) | (int(tick) + 2),
                          (int(dim) << 32) | int(env))
        u1 = max(float(self._u01(w[0])), 1e-12)
        u2 = float(self._u01(w[1]))
        return float(np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2))

    def draw(self, tick: int, n_envs: int, obs_dim: int) -> np.ndarray:
        return np.array([[self.normal(tick, i, k) for k in range(obs_dim)]
                         for i in range(n_envs)])


class VectorSynthetic:
    """M independent SyntheticEnv instances of one spec in float32 numpy
    arrays: s' = tanh(s.W + a.U + proc_sigma.N(0,1)), r = -mean(s'^2) +
    0.1.mean(a^2), fixed horizon.  Takes SyntheticEnv's (obs_dim, act_dim,
    horizon, act_high, seed) and derives W, U with the same default_rng(seed)
    draws, so one seed names one env on both sides; they are exposed as
    float32.  Actions are NORMALIZED to (-1, 1) and scaled by act_high
    inside (the NormalizeAction convention), as in VectorPendulum, and
    episodes are synchronized: done is the scalar horizon flag.

    Host twin of the device synthetic rollout (ops/hip/engine_synth.hip),
    so it serves both as the CPU vector-actor path and as the parity oracle.
    The process noise comes from ``proc_noise``, a replaceable source with
    ``draw(tick, n_envs, obs_dim)`` and ``reset()``: a GeneratorProcNoise by
    default, a PhiloxProcNoise to draw what the kernel draws.  ``seed``
    names the env (W, U); reset states and the default process noise come
    from a Generator seeded with ``noise_seed`` (``seed`` when None, as in
    SyntheticEnv), so a caller that seeds other streams with ``seed`` can
    keep this one apart."""

    def __init__(self, n_envs: int, obs_dim: int, act_dim: int,
                 horizon: int = 1000, act_high: float = 1.0,
                 seed: int | None = None, proc_sigma: float = 0.01,
                 proc_noise=None, noise_seed: int | None = None):
        self.n = int(n_envs)
        self.obs_dim, self.act_dim = int(obs_dim), int(act_dim)
        self.horizon = int(horizon)
        self.act_high = np.float32(act_high)
        self.proc_sigma = np.float32(proc_sigma)
        self.rng = np.random.default_rng(
            seed if noise_seed is None else noise_seed)
        mix_rng = np.random.default_rng(0 if seed is None else seed)
        a = (mix_rng.standard_normal((self.obs_dim, self.obs_dim))
             / np.sqrt(self.obs_dim))
        self.W = (0.9 * a).astype(np.float32)
        self.U = (mix_rng.standard_normal((self.act_dim, self.obs_dim))
                  / np.sqrt(self.act_dim)).astype(np.float32)
        self.proc_noise = (GeneratorProcNoise(self.rng) if proc_noise is None
                           else proc_noise)
        self.state = np.zeros((self.n, self.obs_dim), np.float32)
        self.t = 0

    def set_state(self, state) -> np.ndarray:
        """Start an episode from the given states."""
        self.state = np.array(state, np.float32).reshape(self.n,
                                                         self.obs_dim)
        self.t = 0
        return self.state.copy()

    def reset(self) -> np.ndarray:
        self.proc_noise.reset()
        return self.set_state(
            0.1 * self.rng.standard_normal((self.n, self.obs_dim)))

    def step(self, actions: np.ndarray):
        """actions [M, act_dim] in (-1, 1).  Returns (obs, rewards, done)
        where done is a scalar — the synchronized horizon flag."""
        f = np.float32
        u = np.clip(np.asarray(actions, f).reshape(self.n, self.act_dim),
                    f(-1.0), f(1.0)) * self.act_high
        z = self.state @ self.W + u @ self.U
        if self.proc_sigma != 0:
            noise = self.proc_noise.draw(self.t, self.n, self.obs_dim)
            z = z + self.proc_sigma * np.asarray(noise).astype(f)
        self.state = np.tanh(z).astype(f)
        reward = (-np.mean(self.state ** 2, axis=1)
                  + f(0.1) * np.mean(u ** 2, axis=1)).astype(f)
        self.t += 1
        return self.state.copy(), reward, self.t >= self.horizon


def vector_evaluate(actor, vec_env, episodes: int = 1, reset: bool = True):
    """Greedy evaluation over a vector env: ``episodes`` noise-free episodes
    of all ``vec_env.n`` envs under ``actor`` (a torch module mapping
    [M, obs] to [M, act], or an agent holding one as ``.actor``), the action
    being clip(actor(obs), -1, 1).  Dynamics are the twins' own float32
    update order; the undiscounted returns are summed in float64 in tick
    order.

    Returns ``(summary, (ret, len, succ))``: summary is the dict
    ``FusedEngine.evaluate`` returns (mean_return, min_return, max_return,
    success_rate, env_steps, episodes) over all env episodes of the call, and
    the arrays are per env for the LAST episode (float64, int32, int32).
    Host twin of the device evaluation (ops/hip/engine_eval.hip): it is what
    the CPU path calls, and the device path's parity oracle when the env's
    start states and process noise come from the philox sources.

    ``reset=False`` starts the first episode from the state the env already
    holds (after ``set_state``, or th / thdot / t set by hand), which is how
    the tests inject start states; later episodes always reset."""
    import torch

    if isinstance(vec_env, VectorGoalReach):
        kind = "goal"
    elif isinstance(vec_env, (VectorPendulum, VectorSynthetic)):
        kind = "sync"
    else:
        raise TypeError(
            "vector_evaluate: unsupported vector env %s (VectorPendulum, "
            "VectorGoalReach or VectorSynthetic)" % type(vec_env).__name__)
    episodes = int(episodes)
    if episodes < 1:
        raise ValueError("vector_evaluate: episodes < 1")
    net = getattr(actor, "actor", actor)
    m, horizon = vec_env.n, vec_env.horizon

    def policy(obs):
        with torch.no_grad():
            a = net(torch.from_numpy(np.ascontiguousarray(obs, np.float32)))
        return np.clip(a.numpy(), -1.0, 1.0).astype(np.float32)

    total = 0.0
    lo, hi = np.inf, -np.inf
    n_succ = n_steps = 0
    for ep in range(episodes):
        if reset or ep > 0:
            obs = vec_env.reset()
        elif isinstance(vec_env, VectorSynthetic):
            obs = vec_env.state.copy()
        else:
            obs = vec_env._obs()
        ret = np.zeros(m, np.float64)
        succ = np.zeros(m, np.int32)
        if kind == "goal":
            for _ in range(horizon):
                live = vec_env.alive.copy()
                if not live.any():
                    break
                obs, r, _, _ = vec_env.step(policy(obs))
                ret[live] += r[live].astype(np.float64)
            length = vec_env.len.astype(np.int32)
            succ = vec_env.succ.astype(np.int32)
        else:
            for _ in range(horizon):
                obs, r, _ = vec_env.step(policy(obs))
                ret += np.asarray(r, np.float64)
            length = np.full(m, horizon, np.int32)
        total += float(np.sum(ret, dtype=np.float64))
        lo, hi = min(lo, float(ret.min())), max(hi, float(ret.max()))
        n_succ += int(succ.sum())
        n_steps += int(length.sum())
    count = m * episodes
    summary = dict(mean_return=total / count, min_return=lo, max_return=hi,
                   success_rate=n_succ / count, env_steps=n_steps,
                   episodes=episodes)
    return summary, (ret, length, succ)
