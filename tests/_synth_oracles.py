"""Oracles for the synthetic-spec rollout (ops/hip/engine_synth.hip): its
philox streams value by value, and whole episodes of the host twin
(VectorSynthetic + VecNStep) driven by a torch actor and those streams.
Shared by the CPU and GPU tests; builds on _oracles.py."""

from __future__ import annotations

import copy

import numpy as np
import torch

import _oracles as orc

RESET_STREAM = 0xD011E
ACT_STREAM = 0x2F01E
PROC_STREAM = 0x51A7E


def _ctr_lo(env, dim):
    return (int(dim) << 32) | int(env)


def reset_state(seed, ep, m, obs_dim):
    """[m, obs_dim] float32 state the device reset gives at episode `ep`:
    0.1f * n01 of the first two words, dim k of env i at ctr_lo (k << 32)
    | i."""
    out = np.zeros((m, obs_dim), np.float32)
    for i in range(m):
        for k in range(obs_dim):
            v = orc.philox4x32_10(int(seed) ^ RESET_STREAM,
                                  (int(ep) << 20) | 1, _ctr_lo(i, k))
            out[i, k] = np.float32(0.1) * np.float32(orc.n01(v[0], v[1]))
    return out


def act_normal(seed, ep, tick, env, dim):
    v = orc.philox4x32_10(int(seed) ^ ACT_STREAM,
                          (int(ep) << 20) | (tick + 2), _ctr_lo(env, dim))
    return orc.n01(v[0], v[1])


def act_normals(seed, ep, tick, m, act_dim):
    """[m, act_dim] float64 standard normals of the exploration stream."""
    return np.array([[act_normal(seed, ep, tick, i, k)
                      for k in range(act_dim)] for i in range(m)])


def proc_normal(seed, ep, tick, env, dim):
    v = orc.philox4x32_10(int(seed) ^ PROC_STREAM,
                          (int(ep) << 20) | (tick + 2), _ctr_lo(env, dim))
    return orc.n01(v[0], v[1])


def proc_normals(seed, ep, tick, m, obs_dim):
    return np.array([[proc_normal(seed, ep, tick, i, k)
                      for k in range(obs_dim)] for i in range(m)])


class Exploration:
    """The device's exploration noise as a per-tick [m, act_dim] float64
    additive term: eps * N(0,1) (gaussian) or eps * x with the OU recurrence
    x += theta (mu - x) dt + sigma sqrt(dt) N(0,1), x0 = mu, dt = 1e-2."""

    def __init__(self, m, act_dim, seed, ep, kind="gaussian", eps=0.3,
                 ou_theta=0.15, ou_sigma=0.2, ou_mu=0.0):
        self.m, self.a, self.seed, self.ep = m, act_dim, seed, ep
        self.kind, self.eps = kind, float(np.float32(eps))
        self.theta, self.sigma = float(np.float32(ou_theta)), \
            float(np.float32(ou_sigma))
        self.mu, self.dt = float(np.float32(ou_mu)), float(np.float32(1e-2))
        self.x = np.full((m, act_dim), self.mu)

    def __call__(self, tick):
        if self.kind == "gaussian":
            if self.eps == 0.0:
                return np.zeros((self.m, self.a))
            return self.eps * act_normals(self.seed, self.ep, tick, self.m,
                                          self.a)
        g = act_normals(self.seed, self.ep, tick, self.m, self.a)
        self.x = (self.x + self.theta * (self.mu - self.x) * self.dt
                  + self.sigma * np.sqrt(self.dt) * g)
        return self.eps * self.x


def twin_episode(net, vec, fold, state0, explore):
    """One episode of the float32 host twin from `state0`: the torch actor,
    the exploration term, VectorSynthetic.step and the VecNStep fold.
    Returns the rows (S, A, R, S2, D) in emit order and the per-tick
    normalized actions [horizon, M, A]."""
    obs = vec.set_state(state0)
    fold.reset()
    rows, acts = [], []
    with torch.no_grad():
        for t in range(vec.horizon):
            a = net(torch.from_numpy(obs)).numpy().astype(np.float64)
            a = np.clip(a + explore(t), -1.0, 1.0).astype(np.float32)
            acts.append(a)
            obs2, r, done = vec.step(a)
            out = fold.push(obs, a, r, obs2, done)
            if out is not None:
                rows.append(out)
            obs = obs2
    assert done
    return (tuple(np.concatenate([b[j] for b in rows]) for j in range(5)),
            np.stack(acts))


def f64_episode(net, W, U, state0, explore, *, n, horizon, gamma, act_high,
                proc_sigma, proc_seed=None, ep=1):
    """The same recurrence in float64 throughout (actor included), written
    out directly: the reference the float32 twin's own rounding is measured
    against.  W, U are the float32 matrices widened."""
    net64 = copy.deepcopy(net).double()
    W, U = np.asarray(W, np.float64), np.asarray(U, np.float64)
    m, o = np.shape(state0)
    s = np.asarray(state0, np.float64)
    hist_s, hist_a, hist_r = [], [], []
    S, A, R, S2, D = [], [], [], [], []
    with torch.no_grad():
        for t in range(horizon):
            a = net64(torch.from_numpy(s)).numpy()
            a = np.clip(a + explore(t), -1.0, 1.0)
            u = a * float(np.float32(act_high))
            z = s @ W + u @ U
            if proc_sigma:
                z = z + float(np.float32(proc_sigma)) * proc_normals(
                    proc_seed, ep, t, m, o)
            s2 = np.tanh(z)
            r = -np.mean(s2 ** 2, axis=1) + 0.1 * np.mean(u ** 2, axis=1)
            hist_s.append(s), hist_a.append(a), hist_r.append(r)
            if t >= n - 1:
                t0 = t - n + 1
                S.append(hist_s[t0]), A.append(hist_a[t0]), S2.append(s2)
                R.append(sum(float(np.float32(gamma)) ** k * hist_r[t0 + k]
                             for k in range(n)))
                D.append(np.full(m, float(t == horizon - 1)))
            s = s2
    return tuple(np.concatenate(x) for x in (S, A, R, S2, D))


def max_dev(rows_a, rows_b):
    """Largest absolute difference over s, a, r, s2 of two row sets."""
    return max(float(np.abs(np.asarray(x, np.float64)
                            - np.asarray(y, np.float64)).max())
               for x, y in list(zip(rows_a, rows_b))[:4])
