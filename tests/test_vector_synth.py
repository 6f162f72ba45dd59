"""CPU tests of the vectorized synthetic-spec actor: VectorSynthetic against
scalar SyntheticEnv instances, its philox process-noise source against the
test oracle, the VecNStep pairing, and the --vector_envs wiring of actor
ranks for Synthetic envs."""

import os

import numpy as np
import pytest
import torch.multiprocessing as mp

import _synth_oracles as so
from d4pg_amd.envs import NormalizeAction
from d4pg_amd.envs.synthetic import SyntheticEnv
from d4pg_amd.envs.vector import (SYNTH_PROC_STREAM, PhiloxProcNoise,
                                  VecNStep, VectorSynthetic)

M = 4
SEED = 11


class _FixedNoise:
    """Process-noise source handing out prepared values [tick][M][O]."""

    def __init__(self, values):
        self.values = values

    def reset(self):
        pass

    def draw(self, tick, n_envs, obs_dim):
        return self.values[tick]


class _FixedRng:
    """Stands in for a scalar env's Generator: standard_normal returns the
    prepared rows one after the other."""

    def __init__(self, rows):
        self.rows = list(rows)

    def standard_normal(self, size):
        row = self.rows.pop(0)
        assert np.shape(row) == (size,)
        return row


def _run_both(o, a, act_high, steps=10, horizon=1000):
    rng = np.random.default_rng(o * 100 + a)
    noise = rng.standard_normal((steps, M, o))
    state0 = 0.1 * rng.standard_normal((M, o))
    # some actions outside (-1, 1): the clip is part of the contract
    actions = rng.uniform(-1.2, 1.2, (steps, M, a)).astype(np.float32)
    vec = VectorSynthetic(M, o, a, horizon=horizon, act_high=act_high,
                          seed=SEED, proc_noise=_FixedNoise(noise))
    obs = vec.set_state(state0)
    assert obs.dtype == np.float32 and obs.shape == (M, o)
    envs = []
    for i in range(M):
        env = SyntheticEnv(o, a, horizon=horizon, act_high=act_high,
                           seed=SEED)
        env.reset()
        env.state = state0[i].astype(np.float32).astype(np.float64)
        env.rng = _FixedRng(noise[:, i])
        envs.append(NormalizeAction(env))
    out = []
    for t in range(steps):
        obs, r, done = vec.step(actions[t])
        want_s = np.zeros((M, o))
        want_r = np.zeros(M)
        for i, env in enumerate(envs):
            s_i, r_i, _, _ = env.step(np.clip(actions[t, i], -1.0, 1.0))
            want_s[i], want_r[i] = env.wrapped.state, r_i
        out.append((obs, r, done, want_s, want_r))
    return vec, envs, actions, out


@pytest.mark.parametrize("o,a", [(5, 2), (17, 6), (376, 17)])
def test_vector_synthetic_matches_scalar_envs(o, a):
    vec, envs, _, out = _run_both(o, a, act_high=1.0)
    ref = envs[0].wrapped
    assert vec.W.dtype == np.float32 and vec.U.dtype == np.float32
    assert np.array_equal(vec.W, ref.W.astype(np.float32))
    assert np.array_equal(vec.U, ref.U.astype(np.float32))
    worst_s = worst_r = 0.0
    for obs, r, done, want_s, want_r in out:
        assert obs.dtype == np.float32 and r.dtype == np.float32
        assert not done
        worst_s = max(worst_s, np.abs(obs - want_s).max())
        worst_r = max(worst_r, np.abs(r - want_r).max())
    print(f"({o}, {a}): max abs err state {worst_s:.3g} reward {worst_r:.3g}")
    assert worst_s <= 1e-5 and worst_r <= 1e-5


def test_act_high_scales_the_action_inside():
    """With W = 0 the next state is tanh(act_high * a . U) and the reward's
    action term is 0.1 * act_high^2 * mean(a^2)."""
    o, a, hi = 5, 2, 0.4
    vec, envs, actions, out = _run_both(o, a, act_high=hi, steps=3)
    for obs, r, _, want_s, want_r in out:
        assert np.abs(obs - want_s).max() <= 1e-5
        assert np.abs(r - want_r).max() <= 1e-5
    one = VectorSynthetic(M, o, a, act_high=1.0, seed=SEED, proc_sigma=0.0)
    sc = VectorSynthetic(M, o, a, act_high=hi, seed=SEED, proc_sigma=0.0)
    for v in (one, sc):
        v.W[:] = 0.0
        v.set_state(np.zeros((M, o)))
    act = np.clip(actions[0], -1.0, 1.0)
    s1, r1, _ = one.step(act)
    s2, r2, _ = sc.step(act)
    mix = act.astype(np.float64) @ one.U.astype(np.float64)
    np.testing.assert_allclose(s1, np.tanh(mix), rtol=0, atol=1e-6)
    np.testing.assert_allclose(s2, np.tanh(float(np.float32(hi)) * mix),
                               rtol=0, atol=1e-6)
    a_term = 0.1 * np.mean(act.astype(np.float64) ** 2, axis=1)
    np.testing.assert_allclose(r1 + np.mean(s1 ** 2, axis=1), a_term,
                               rtol=0, atol=1e-6)
    np.testing.assert_allclose(r2 + np.mean(s2 ** 2, axis=1),
                               hi * hi * a_term, rtol=0, atol=1e-6)


def test_done_exactly_at_horizon():
    vec = VectorSynthetic(M, 5, 2, horizon=4, seed=SEED)
    vec.reset()
    flags = [vec.step(np.zeros((M, 2), np.float32))[2] for _ in range(4)]
    assert flags == [False, False, False, True]
    obs = vec.reset()
    assert vec.t == 0 and np.abs(obs).max() < 1.0 and np.abs(obs).max() > 0
    assert vec.step(np.zeros((M, 2), np.float32))[2] is False


def test_noise_seed_keeps_the_env_and_moves_the_streams():
    """`seed` names W, U; `noise_seed` seeds reset states and process noise,
    so a caller drawing its exploration noise from default_rng(seed) does
    not replay the twin's own draws."""
    same = VectorSynthetic(M, 5, 2, seed=SEED)
    apart = VectorSynthetic(M, 5, 2, seed=SEED, noise_seed=SEED + 17)
    assert np.array_equal(same.W, apart.W) and np.array_equal(same.U, apart.U)
    caller = np.random.default_rng(SEED)
    first = (0.1 * caller.standard_normal((M, 5))).astype(np.float32)
    assert np.array_equal(same.reset(), first)      # SyntheticEnv's default
    r = apart.reset()
    assert not np.isin(r, first).any()
    want = (0.1 * np.random.default_rng(SEED + 17).standard_normal((M, 5))
            ).astype(np.float32)
    assert np.array_equal(r, want)


def test_library_philox_source_is_the_oracle_philox():
    assert SYNTH_PROC_STREAM == so.PROC_STREAM
    src = PhiloxProcNoise(seed=77, episode=2)
    got = src.draw(3, 5, 7)
    want = so.proc_normals(77, 2, 3, 5, 7)
    assert got.shape == (5, 7) and np.array_equal(got, want)
    assert len(np.unique(got)) == 35            # every (env, dim) its own
    assert src.normal(0, 4, 6) == so.proc_normal(77, 2, 0, 4, 6)
    src.reset()                                 # next episode, as the device
    assert np.array_equal(src.draw(3, 2, 2), so.proc_normals(77, 3, 3, 2, 2))
    # the source plugs into the twin: W = U = 0 reads the draw off
    vec = VectorSynthetic(2, 3, 1, seed=SEED, proc_sigma=0.5,
                          proc_noise=PhiloxProcNoise(77, 1))
    vec.W[:] = 0.0
    vec.U[:] = 0.0
    vec.set_state(np.zeros((2, 3)))
    s, _, _ = vec.step(np.zeros((2, 1), np.float32))
    np.testing.assert_allclose(
        s, np.tanh(0.5 * so.proc_normals(77, 1, 0, 2, 3)), rtol=0, atol=1e-6)


@pytest.mark.parametrize("n", [1, 3])
def test_vecnstep_pairing_row_count_and_done(n):
    hor, o, a = 7, 5, 2
    vec = VectorSynthetic(M, o, a, horizon=hor, seed=SEED)
    fold = VecNStep(M, o, a, n, 0.99)
    rng = np.random.default_rng(0)
    obs = vec.reset()
    rows, rewards, states = [], [], [obs]
    for t in range(hor):
        act = rng.uniform(-1, 1, (M, a)).astype(np.float32)
        obs2, r, done = vec.step(act)
        out = fold.push(obs, act, r, obs2, done)
        if out is not None:
            rows.append(out)
        rewards.append(r)
        states.append(obs2)
        obs = obs2
    S, A, R, S2, D = (np.concatenate([b[j] for b in rows]) for j in range(5))
    assert len(R) == M * (hor - n + 1)
    assert (D[:-M] == 0).all() and (D[-M:] == 1).all()
    assert np.array_equal(S[:M], states[0]) and np.array_equal(S2[-M:],
                                                               states[-1])
    want_R = sum(0.99 ** k * rewards[k].astype(np.float64) for k in range(n))
    np.testing.assert_allclose(R[:M], want_R, rtol=0, atol=1e-6)


# ---------------------------------------------------------------------------
# two-rank gloo run: the actor rank takes the vector path
# ---------------------------------------------------------------------------

def _rank_main(rank, world, port, extra, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["RANK"] = str(rank)
    os.environ["WORLD_SIZE"] = str(world)
    import torch.distributed as dist
    from d4pg_amd.parallel.learner import DistributedD4PG
    from test_distributed import _mk_args
    dist.init_process_group("gloo", rank=rank, world_size=world)
    node = DistributedD4PG(_mk_args(extra), rank=rank, world=world,
                           device="cpu")
    step = node.run(rounds=4)
    if rank == 0:
        q.put(("learner", step, len(node.agent.replayBuffer), None))
    else:
        q.put((f"rank{rank}", step, node.env_meter.count,
               (type(node.vector).__name__, node.vector.n,
                node.vector.obs_dim, node.vector.act_dim, node.push_cap)))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_vector_synth_actor():
    """--env Synthetic-5x2 --vector_envs 8: the actor rank collects with
    VectorSynthetic + VecNStep and the learner trains."""
    extra = ("--env", "Synthetic-5x2", "--vector_envs", "8",
             "--max_steps", "20")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_main, args=(r, 2, 29651, extra, q))
             for r in range(2)]
    for p in procs:
        p.start()
    out = {}
    for _ in range(2):
        tag, step, x, path = q.get(timeout=300)
        out[tag] = (step, x, path)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    step, replay_len, _ = out["learner"]
    _, env_steps, path = out["rank1"]
    assert path == ("VectorSynthetic", 8, 5, 2, 8 * 20)
    # 4 rounds x 8 envs x (20 - 3 + 1) folded rows, one episode per round
    assert replay_len == 4 * 8 * 18
    assert env_steps == 4 * 8 * 20
    assert step > 0
