"""Host twins of the device goal-reaching rollout (ops/hip/engine_goal.hip):
the oracle episode, the searched start states, the HER draws, the margin
condition and the emit-order rows.  Shared by test_gpu_goal_rollout.py and
test_gpu_uniform_replay.py; the tests and their bounds live there.
"""

import functools

import numpy as np
import torch

import _engine_kit as kit
import _oracles as orc
from d4pg_amd.envs.vector import VectorGoalReach
from d4pg_amd.her import HER_STREAM, PhiloxHerRng, vector_add_experience

D = 2
O, A, H, K = 2 * D, D, 256, 51
DIST = {"type": "categorical", "v_min": -50.0, "v_max": 0.0, "n_atoms": K}
M, HOR = 8, 10
SPEED, TOL, EPS, GAMMA = 0.1, 0.3, 0.3, 0.99
SEED = 77                               # rollout seed (noise, reset, HER)
NET_SEED = 4
ALPHA = np.float64(np.float32(0.6))     # the engine holds per_alpha as float
MARGIN = 1e-3


def _nets(critic_seed):
    return kit.producer_nets(O, A, DIST, hidden=H, actor_seed=NET_SEED,
                             critic_seed=critic_seed)


@functools.lru_cache(maxsize=None)
def net():
    return _nets(0)[0]


def make_engine(capacity, seed=0, batch=64, prioritized=True):
    """The critic is seeded with the engine's seed."""
    return kit.producer_engine(
        O, A, hidden=H, n_atoms=K, capacity=capacity, batch=batch, seed=seed,
        v_min=-50.0, v_max=0.0, gamma_n=GAMMA ** 3, lr=1e-4,
        prioritized=prioritized, actor_seed=NET_SEED, critic_seed=seed)[0]


def episode_max(m, n, hor):
    return m * (hor - n + 1) + m * hor


def _noise(seed, ep, tick, m, eps):
    """eps * N(0,1) for every env and action dim at `tick`: dim k of env i
    draws with ctr_lo = (k << 32) | i."""
    return np.array([[eps * orc.n01(*orc.roll_noise_words(
        seed, ep, tick, (k << 32) | i)[:2]) for k in range(D)]
        for i in range(m)])


def cpu_episode(pos0, goal0, eps, seed=SEED, ep=1, hor=HOR, tol=TOL):
    """Oracle episode: VectorGoalReach + the torch actor + philox noise."""
    m = len(pos0)
    vec = VectorGoalReach(m, dim=D, speed=SPEED, tol=tol, horizon=hor)
    obs = vec.set_state(pos0, goal0)
    with torch.no_grad():
        for t in range(hor):
            a = net()(torch.from_numpy(obs)).numpy().astype(np.float64)
            if eps:
                a = a + _noise(seed, ep, t, m, eps)
            obs, _, _, _ = vec.step(np.clip(a, -1.0, 1.0).astype(np.float32))
    return vec


@functools.lru_cache(maxsize=None)
def starts():
    """(pos, goal) for the M envs, chosen with the oracle so that the
    episode lengths include 1, 2 (< n for n = 3), a mid value and HOR (no
    success).  Envs are independent given their index (per-row policy,
    per-env noise stream), so slot i is searched on its own over passes of
    candidate starts."""
    want = [1, 2, 5, HOR, None, None, 1, None]     # None: take pass 0
    rng = np.random.default_rng(5)
    pos = np.zeros((M, D), np.float32)
    goal = np.zeros((M, D), np.float32)
    found = [False] * M
    for p in range(60):
        c_pos = rng.uniform(-0.4, 0.4, (M, D)).astype(np.float32)
        ang = rng.uniform(0, 2 * np.pi, M)
        dist = rng.choice([0.31, 0.33, 0.36, 0.4, 0.45, 1.3], M)
        c_goal = (c_pos + (dist * np.stack([np.cos(ang), np.sin(ang)])).T
                  ).astype(np.float32)
        c_goal = np.clip(c_goal, -1.0, 1.0)
        vec = cpu_episode(c_pos, c_goal, EPS)
        for i in range(M):
            T, ok = int(vec.len[i]), bool(vec.succ[i])
            hit = (want[i] is None or
                   (want[i] == HOR and T == HOR and not ok) or
                   (want[i] == 5 and 3 <= T < HOR and ok) or
                   (want[i] in (1, 2) and T == want[i] and ok))
            if hit and not found[i]:
                pos[i], goal[i], found[i] = c_pos[i], c_goal[i], True
        if all(found):
            break
    assert all(found), f"no start found for slots {found}"
    return pos, goal


def _her_draw(seed, ep, t, i, T, ratio):
    w = orc.philox4x32_10(seed ^ HER_STREAM, (ep << 20) | t, i)
    hit = ratio > 0 and orc.u01(w[0]) <= np.float32(ratio)
    return hit, t + w[1] % (T - t)


def env_margins(ep_pos, length, goal, ratio, seed=SEED, ep=1, tol=TOL):
    """Per env, the least |d - tol| over the real and the hindsight
    distances of a recorded episode (fut == t ones, exactly 0, left out)."""
    out = np.full(len(length), np.inf)
    for i in range(len(length)):
        T = int(length[i])
        for t in range(T):
            p = ep_pos[t + 1, i].astype(np.float64)
            ds = [np.linalg.norm(p - goal[i])]
            hit, fut = _her_draw(seed, ep, t, i, T, ratio)
            if hit and fut != t:
                ds.append(np.linalg.norm(p - ep_pos[fut + 1, i]))
            out[i] = min(out[i], min(abs(d - tol) for d in ds))
    return out


def assert_margin(ep_pos, length, goal, ratio, seed=SEED, ep=1, tol=TOL):
    """The margin condition of the module docstring."""
    worst = env_margins(ep_pos, length, goal, ratio, seed, ep, tol).min()
    assert worst > MARGIN, (
        f"misconfigured test: a distance is {worst:.2e} from tol")
    return worst


class _Rows:
    def __init__(self):
        self.s, self.a, self.r, self.s2, self.d = [], [], [], [], []

    def add(self, s, a, r, s2, d):
        self.s.append(np.asarray(s, np.float32))
        self.a.append(np.asarray(a, np.float32))
        self.r.append(np.float32(r))
        self.s2.append(np.asarray(s2, np.float32))
        self.d.append(np.float32(d))

    def arrays(self):
        return (np.stack(self.s).reshape(-1, O), np.stack(self.a).reshape(-1, A),
                np.asarray(self.r, np.float32), np.stack(self.s2).reshape(-1, O),
                np.asarray(self.d, np.float32))


def oracle_rows(epi, n, ratio, seed=SEED, ep=1, tol=TOL):
    """vector_add_experience over a recorded episode, with the device's HER
    draws: (S, A, R, S2, D) in the device's emit order."""
    m = len(epi["len"])
    env = VectorGoalReach(m, dim=D, speed=SPEED, tol=tol, horizon=1)
    rows = _Rows()
    n_rows = vector_add_experience(
        rows, env, epi["ep_pos"], epi["ep_act"], epi["len"], epi["succ"],
        epi["goal"], her=True, her_ratio=ratio, n_steps=n, gamma=GAMMA,
        rng=lambda i: PhiloxHerRng(seed, ep, i))
    out = rows.arrays()
    assert n_rows == len(out[2])
    return out


def oracle_counts(epi, n, ratio, seed=SEED, ep=1):
    out = []
    for i, T in enumerate(int(x) for x in epi["len"]):
        hits = sum(_her_draw(seed, ep, t, i, T, ratio)[0] for t in range(T))
        out.append(max(0, T - n + 1) + hits)
    return np.asarray(out, np.int64)


def device_episode(eng):
    return {k: v.numpy() for k, v in eng.goal_rollout_episode().items()}


def assert_rows_equal(got, want, n):
    """s, a, s2 are copies: bitwise.  r: bitwise for n = 1, rtol 1e-6 for
    the folded sums.  d: equal."""
    s, a, r, s2, d = got
    S, Aa, R, S2, Dn = want
    assert len(r) == len(R)
    assert np.array_equal(s, S) and np.array_equal(s2, S2)
    assert np.array_equal(a, Aa)
    if n == 1:
        assert np.array_equal(r, R)
    else:
        np.testing.assert_allclose(r, R, rtol=1e-6, atol=0)
    assert np.array_equal(d, Dn)
