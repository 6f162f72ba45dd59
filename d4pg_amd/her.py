"""Hindsight Experience Replay (HER) relabeling + episode collection.

Capability parity with /root/reference/main.py:137-185
(``addExperienceToBuffer``): roll one episode with exploration noise, then
write transitions with goal-concatenated observations; with HER enabled,
each timestep additionally (with probability ``her_ratio``) stores a
hindsight copy relabeled to a future achieved goal, reward recomputed via
``env.compute_reward``, done set when the recomputed reward is 0.

Fixed deviations (SURVEY.md §7 quirk list):
  * the reference's hindsight transition stores the loop-final ``action``
    variable instead of the timestep's action (main.py:184, known bug) —
    fixed here: the relabeled tuple carries ``episode[t]``'s action;
  * the reference only writes to the buffer at all when HER is on
    (``if args.her and not done`` guards the entire add-loop, main.py:154,
    so ``--her 0`` never trains) — here non-HER episodes are stored too,
    which is what the reference's commented-out code intended.

n-step note: the reference applies n-step folding only in the separate
Worker warmup path (main.py:224-234), not in HER adds; here both paths fold
through the same NStepFolder for consistency.
"""

from __future__ import annotations

import numpy as np

from .replay.nstep import NStepFolder


def flat_obs(o):
    """Goal-concat for dict observations (reference main.py:144 semantics),
    identity for flat ones."""
    if isinstance(o, dict):
        return np.concatenate([np.asarray(o["observation"], np.float32).ravel(),
                               np.asarray(o["desired_goal"], np.float32).ravel()])
    return np.asarray(o, np.float32).ravel()


def rollout_episode(policy, env, noise=True, max_steps=None):
    """Collect one episode.  Returns (episode, total_reward, success) where
    episode is a list of (obs, action, reward, next_obs, done, info) with
    raw (possibly dict) observations."""
    episode = []
    obs = env.reset()
    total_r = 0.0
    success = False
    steps = max_steps or env._max_episode_steps
    for _ in range(steps):
        a = policy.select_action(flat_obs(obs), explore=noise)
        next_obs, r, done, info = env.step(a)
        if isinstance(info, dict) and "is_success" in info:
            done = bool(info["is_success"]) or done
            success = success or bool(info["is_success"])
        episode.append((obs, a, r, next_obs, done, info))
        total_r += r
        obs = next_obs
        if done:
            break
    return episode, total_r, success


def add_experience(replay_buffer, env, episode, her: bool = False,
                   her_ratio: float = 0.8, n_steps: int = 1,
                   gamma: float = 0.99,
                   rng: np.random.Generator | None = None) -> int:
    """Store an episode's transitions (+ optional HER relabels).
    Returns the number of tuples written."""
    rng = rng or np.random.default_rng()
    written = 0

    folder = NStepFolder(n_steps, gamma)
    for (obs, a, r, next_obs, done, info) in episode:
        for tr in folder.push(flat_obs(obs), a, r, flat_obs(next_obs), done):
            replay_buffer.add(*tr)
            written += 1

    if her and episode and isinstance(episode[0][0], dict):
        T = len(episode)
        her_folder = NStepFolder(1, gamma)  # relabeled tuples are 1-step
        for t, (obs, a, r, next_obs, done, info) in enumerate(episode):
            if rng.random() >= her_ratio:
                continue
            # "future" strategy: substitute an achieved goal from t..T-1
            fut = int(rng.integers(t, T))
            new_goal = np.asarray(episode[fut][3]["achieved_goal"])
            achieved = np.asarray(next_obs["achieved_goal"])
            new_r = float(np.asarray(env.compute_reward(achieved, new_goal)))
            new_done = new_r == 0.0
            s = np.concatenate([np.asarray(obs["observation"],
                                           np.float32).ravel(),
                                new_goal.astype(np.float32).ravel()])
            s2 = np.concatenate([np.asarray(next_obs["observation"],
                                            np.float32).ravel(),
                                 new_goal.astype(np.float32).ravel()])
            replay_buffer.add(s, a, new_r, s2, new_done)   # a = this step's
            written += 1
        del her_folder
    return written


# ---------------------------------------------------------------------------
# vectorized goal episodes (VectorGoalReach / the device goal rollout)
# ---------------------------------------------------------------------------

_PHILOX_M0, _PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_U32 = 0xFFFFFFFF

# seed-xor constant of the device HER stream (engine_goal.hip goal_her_draw)
HER_STREAM = 0x4E12E


def philox4x32_10(seed: int, ctr_hi: int, ctr_lo: int):
    """philox4x32-10 in the engine's calling convention: 64-bit seed -> key,
    ctr_lo -> counter words 0,1 and ctr_hi -> counter words 2,3."""
    seed, ctr_hi, ctr_lo = int(seed), int(ctr_hi), int(ctr_lo)
    c0, c1 = ctr_lo & _U32, (ctr_lo >> 32) & _U32
    c2, c3 = ctr_hi & _U32, (ctr_hi >> 32) & _U32
    k0, k1 = seed & _U32, (seed >> 32) & _U32
    for _ in range(10):
        p0, p1 = _PHILOX_M0 * c0, _PHILOX_M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0, p1 & _U32,
                          (p0 >> 32) ^ c3 ^ k1, p0 & _U32)
        k0, k1 = (k0 + _PHILOX_W0) & _U32, (k1 + _PHILOX_W1) & _U32
    return c0, c1, c2, c3


class PhiloxHerRng:
    """The ``rng`` add_experience needs, drawing what the device relabel
    draws for env ``env`` of rollout episode ``episode``: the t-th call of
    ``random()`` takes one philox draw keyed by (seed ^ HER_STREAM,
    (episode << 20) | t, env); the following ``integers(t, T)`` returns
    ``t + w1 % (T - t)`` from the same draw.

    The kernel hits when ``u <= her_ratio`` with u in (0, 1] float32;
    add_experience skips when ``random() >= her_ratio``.  ``random()``
    returns the float32 just below u, so for a float32-representable ratio
    the two tests agree on every draw (vector_add_experience rounds the
    ratio to float32 before passing it on)."""

    def __init__(self, seed: int, episode: int, env: int):
        self.seed, self.episode, self.env = int(seed), int(episode), int(env)
        self._t = -1
        self._w = None

    def random(self) -> float:
        self._t += 1
        self._w = philox4x32_10(self.seed ^ HER_STREAM,
                                (self.episode << 20) | self._t, self.env)
        u = np.float32(np.float32(np.float32(self._w[0]) + np.float32(1.0))
                       * np.float32(2.3283064e-10))
        return float(np.nextafter(u, np.float32(0.0)))

    def integers(self, low: int, high: int) -> int:
        return int(low) + self._w[1] % (int(high) - int(low))


def vector_add_experience(replay_buffer, env, ep_pos, ep_act, length, succ,
                          goal, her: bool = True, her_ratio: float = 0.8,
                          n_steps: int = 1, gamma: float = 0.99,
                          rng=None) -> int:
    """Store the recorded episodes of M vectorized goal envs, in the order
    the device emit writes them: env by env, each env's n-step folded real
    rows by ascending t, then its HER rows by ascending t — i.e. the scalar
    add_experience called once per env.

    ep_pos [>=T+1, M, D], ep_act [>=T, M, D], length [M], succ [M] and
    goal [M, D] are what VectorGoalReach.episode() / the device's
    goal_rollout_episode() record.  ``env`` supplies compute_reward.  Only
    an env's last step, and only when it succeeded, is terminal (the step
    limit is not, as in rollout_episode).  ``rng`` is a numpy Generator
    shared by all envs, or a callable ``env_index -> rng`` (PhiloxHerRng
    for the device's own draws).  Returns the number of rows written."""
    ep_pos = np.asarray(ep_pos, np.float32)
    ep_act = np.asarray(ep_act, np.float32)
    goal = np.asarray(goal, np.float32)
    if rng is None:
        rng = np.random.default_rng()
    ratio = float(np.float32(her_ratio))
    written = 0
    for i in range(ep_pos.shape[1]):
        T = int(length[i])
        g = goal[i]

        def dict_obs(p):
            return {"observation": p, "achieved_goal": p, "desired_goal": g}

        episode = []
        for t in range(T):
            nxt = ep_pos[t + 1, i]
            done = bool(succ[i]) and t == T - 1
            episode.append((dict_obs(ep_pos[t, i]), ep_act[t, i],
                            float(np.asarray(env.compute_reward(nxt, g))),
                            dict_obs(nxt), done, {"is_success": done}))
        written += add_experience(
            replay_buffer, env, episode, her=her, her_ratio=ratio,
            n_steps=n_steps, gamma=gamma,
            rng=rng(i) if callable(rng) else rng)
    return written
