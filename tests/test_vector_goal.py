"""CPU tests of the vectorized goal-reaching actor: VectorGoalReach against
scalar GoalReachEnv instances, vector_add_experience (the scalar
add_experience once per env, with the device's philox HER draws) against a
hand-rolled loop, and the --her_ratio flag."""

import numpy as np
import pytest

import _oracles as orc
from d4pg_amd.envs.goal_reach import GoalReachEnv
from d4pg_amd.envs.vector import VectorGoalReach
from d4pg_amd.her import (HER_STREAM, PhiloxHerRng, philox4x32_10,
                          vector_add_experience)

M, D, HOR = 6, 2, 10
SPEED, TOL = 0.1, 0.05
SEED, EP = 21, 3


def _starts():
    """Starts whose episode lengths under `_policy` are 1 (success on the
    first step), 2 (success on a step < n for n = 3), 6 (mid-episode) and
    HOR without success, plus two envs driven off-axis."""
    pos = np.array([[0.00, 0.00], [-0.50, 0.20], [0.30, -0.60],
                    [-0.90, 0.10], [0.10, 0.10], [0.80, 0.80]], np.float32)
    goal = pos + np.array([[0.08, 0.0], [0.22, 0.0], [0.0, 0.57],
                           [1.60, 0.0], [0.31, -0.23], [-1.5, -1.6]],
                          np.float32)
    return pos, goal


def _policy(obs):
    """Head for the goal, saturating at the action bound."""
    pos, goal = obs[:, :D], obs[:, D:]
    return np.clip((goal - pos) / np.float32(SPEED), -1.0,
                   1.0).astype(np.float32)


@pytest.fixture(scope="module")
def episode():
    pos, goal = _starts()
    vec = VectorGoalReach(M, dim=D, speed=SPEED, tol=TOL, seed=0,
                          horizon=HOR)
    obs = vec.set_state(pos, goal)
    actions = []
    for _ in range(HOR):
        a = _policy(obs)
        actions.append(a)
        obs, _, _, alive = vec.step(a)
    return vec, np.stack(actions)


def test_vector_goal_matches_scalar_envs(episode):
    vec, actions = episode
    pos0, goal = _starts()
    ep_pos, ep_act, length, succ, g = vec.episode()
    assert np.array_equal(g, goal)
    want_len, want_succ = [], []
    for i in range(M):
        env = GoalReachEnv(dim=D, speed=SPEED, tol=TOL, seed=0)
        env.reset()
        env.pos = pos0[i].astype(np.float64)
        env.goal = goal[i].astype(np.float64)
        T, ok = 0, False
        for t in range(HOR):
            o, r, _, info = env.step(actions[t, i])
            T += 1
            d = np.linalg.norm(env.pos - env.goal)
            assert abs(d - TOL) > 1e-3, "start too close to the threshold"
            np.testing.assert_allclose(ep_pos[t + 1, i], env.pos, rtol=0,
                                       atol=1e-6)
            np.testing.assert_array_equal(ep_act[t, i], actions[t, i])
            if info["is_success"]:
                ok = True
                break
        want_len.append(T)
        want_succ.append(ok)
    assert np.array_equal(length, want_len)
    assert np.array_equal(succ, want_succ)
    # the spread the starts were chosen for
    assert list(length[:4]) == [1, 2, 6, HOR]
    assert list(succ[:4]) == [True, True, True, False]


def test_finished_envs_stay_put(episode):
    vec, _ = episode
    ep_pos, _, length, succ, _ = vec.episode()
    assert not vec.alive[succ].any() and vec.alive[~succ].all()
    for i in range(M):
        assert np.array_equal(vec.pos[i], ep_pos[length[i], i])
    with pytest.raises(RuntimeError):
        vec.step(np.zeros((M, D), np.float32))


class _Rows:
    def __init__(self):
        self.rows = []

    def add(self, s, a, r, s2, d):
        self.rows.append((np.asarray(s, np.float32), np.asarray(a, np.float32),
                          np.float32(r), np.asarray(s2, np.float32),
                          np.float32(d)))


def _reward(p, g):
    d = np.linalg.norm(p.astype(np.float64) - g.astype(np.float64))
    return 0.0 if d <= TOL else -1.0


def _hand_rolled(ep_pos, ep_act, length, succ, goal, n, gamma, ratio):
    """Rows in the device order, written out directly: env by env, real
    n-step rows by ascending t, then HER rows by ascending t.  The philox
    is the test oracle's, not the library's."""
    rows, n_her, fut_eq_t = [], [], 0
    ratio32 = np.float32(ratio)
    for i in range(M):
        T, g = int(length[i]), goal[i]
        for t in range(n - 1, T):
            t0 = t - n + 1
            R = sum(gamma ** k * _reward(ep_pos[t0 + k + 1, i], g)
                    for k in range(n))
            rows.append((np.concatenate([ep_pos[t0, i], g]), ep_act[t0, i],
                         np.float32(R), np.concatenate([ep_pos[t + 1, i], g]),
                         np.float32(bool(succ[i]) and t == T - 1)))
        hits = 0
        for t in range(T):
            w = orc.philox4x32_10(SEED ^ 0x4E12E, (EP << 20) | t, i)
            if not (ratio32 > 0 and orc.u01(w[0]) <= ratio32):
                continue
            fut = t + w[1] % (T - t)
            ng = ep_pos[fut + 1, i]
            r = _reward(ep_pos[t + 1, i], ng)
            if fut == t:
                fut_eq_t += 1
                assert r == 0.0
            rows.append((np.concatenate([ep_pos[t, i], ng]), ep_act[t, i],
                         np.float32(r), np.concatenate([ep_pos[t + 1, i], ng]),
                         np.float32(r == 0.0)))
            hits += 1
        n_her.append(hits)
    return rows, n_her, fut_eq_t


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("ratio", [0.0, 0.5, 1.0])
def test_vector_add_experience_matches_hand_rolled(episode, n, ratio):
    vec, _ = episode
    ep_pos, ep_act, length, succ, goal = vec.episode()
    got = _Rows()
    written = vector_add_experience(
        got, vec, ep_pos, ep_act, length, succ, goal, her=True,
        her_ratio=ratio, n_steps=n, gamma=0.99,
        rng=lambda i: PhiloxHerRng(SEED, EP, i))
    want, n_her, fut_eq_t = _hand_rolled(ep_pos, ep_act, length, succ, goal,
                                         n, 0.99, ratio)
    assert written == len(got.rows) == len(want)
    n_real = np.maximum(0, length - n + 1)
    assert written == n_real.sum() + sum(n_her)
    for k, (g, w) in enumerate(zip(got.rows, want)):
        for x, y in zip(g, w):
            np.testing.assert_allclose(x, y, rtol=1e-6, atol=0,
                                       err_msg=f"row {k}")
        assert g[4] == w[4] and (g[2] == w[2] or n > 1)
    if ratio == 0.0:
        assert sum(n_her) == 0
    if ratio == 1.0:
        assert n_her == list(length)
        # the last step of an env can only draw itself
        assert fut_eq_t >= M
    if ratio == 0.5:
        assert 0 < sum(n_her) < length.sum()
    if n == 3:
        # envs 0 and 1 end before the window fills: no real rows, but
        # their steps still get hindsight rows
        assert n_real[0] == 0 and n_real[1] == 0
        if ratio == 1.0:
            assert n_her[0] == 1 and n_her[1] == 2
            first = got.rows[0]
            assert first[2] == 0.0 and first[4] == 1.0    # fut == t
    # done: only a succeeded env's last real row
    pos = 0
    for i in range(M):
        nr = int(n_real[i])
        d = [float(r[4]) for r in got.rows[pos:pos + nr]]
        assert d == [0.0] * (nr - 1) + [float(succ[i])] * min(1, nr)
        pos += nr + n_her[i]


def test_library_philox_is_the_oracle_philox():
    for args in [(0, 0, 0), (SEED ^ HER_STREAM, (EP << 20) | 7, 5),
                 (2 ** 63 + 12345, 2 ** 40 + 3, (1 << 32) | 9)]:
        assert philox4x32_10(*args) == orc.philox4x32_10(*args)


def test_philox_her_rng_hit_test_edges():
    """random() is the float32 just below the kernel's u, so
    `random() >= ratio` (skip) is exactly `not u <= ratio` (the kernel's
    miss), including at u == ratio."""
    rng = PhiloxHerRng(SEED, EP, 2)
    for t in range(50):
        x = rng.random()
        u = orc.u01(orc.philox4x32_10(SEED ^ HER_STREAM, (EP << 20) | t,
                                      2)[0])
        assert x < float(u) and np.float32(x) == np.nextafter(
            u, np.float32(0))
        assert (x >= float(u)) == (not u <= u)          # ratio == u: hit
        below = float(np.nextafter(u, np.float32(0)))
        assert (x >= below) == (not u <= np.float32(below))   # miss
        assert 0.0 <= x < 1.0
        k = rng.integers(t, 60)
        assert t <= k < 60


def test_two_rank_vector_goal_actor():
    """--env GoalReach-v0 --her 1 --vector_envs M: the actor rank collects
    with VectorGoalReach + vector_add_experience and the learner trains."""
    from test_distributed import _run_world
    out = _run_world(2, extra=("--env", "GoalReach-v0", "--her", "1",
                               "--vector_envs", "8", "--max_steps", "20",
                               "--her_ratio", "1.0"), port=29641)
    step, replay_len = out["learner"]
    # 4 rounds x 8 envs x up to (20 - 3 + 1) folded rows + 20 hindsight rows
    assert 4 * 8 * 2 <= replay_len <= 4 * 8 * (18 + 20)
    assert replay_len > 4 * 8 * 18 // 2
    assert step > 0


def test_her_ratio_flag_round_trips():
    from d4pg_amd.config import D4PGConfig, make_parser
    p = make_parser()
    cfg = D4PGConfig.from_args(p.parse_args([]))
    assert cfg.her_ratio == 0.8 and cfg.extra == {}
    cfg = D4PGConfig.from_args(p.parse_args(
        ["--env", "GoalReach-v0", "--her", "1", "--her_ratio", "0.25"]))
    assert cfg.her_ratio == 0.25 and cfg.her == 1 and cfg.extra == {}
