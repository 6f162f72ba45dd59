"""Uniform replay on the fused engine (FusedEngine(prioritized=False)): the
exact integer draw, multi-step determinism, step parity with eager torch, the
absence of the sum/min trees, the write side without leaf writes or tree
sweeps, exact resume and the DDPG wiring.

The draw is philox4x32-10(key=seed, ctr_hi=rng_epoch, ctr_lo=probe), the PER
probe's own stream, mapped to a slot by the integer product of
tests/test_uniform_oracle.py, so every sampled index is compared for
EQUALITY.  Replay sizes here cannot tell a 64-bit product from a 32-bit one;
the CPU oracle test covers the large sizes.
"""

import copy

import numpy as np
import pytest
import torch

import _engine_kit as kit
import _goal_oracles as go
import _oracles as orc
from _oracles import uniform_batch

pytestmark = pytest.mark.gpu

# the shape, replay size and hyper-parameters of test_gpu_multistep.py
O, A, H, K = 5, 2, 128, 51
V_MIN, V_MAX = -300.0, 0.0
GAMMA_N = 0.99 ** 5
TAU, LR = 0.001, 1e-4
N = 512
SEED = 21
BUFFERS = ["sum_tree", "min_tree", "bidx", "pri", "bw", "br", "bd", "ba",
           "bs2", "m_proj", "q"]


def _shape(B, prioritized=False):
    return kit.Shape(B, H, O, A, K, prioritized=prioritized)


def _engine(B, capacity, seed=SEED, prioritized=False, **kw):
    return kit.engine(_shape(B, prioritized), capacity=capacity, seed=seed,
                      **kw)


def _modules(seed=0):
    return kit.modules(_shape(0), seed)


def _transitions(seed=0):
    return kit.transitions(_shape(0), N, seed)


def _rows(rng, T):
    return kit.draw_rows(rng, O, A, T, p_done=0.3)


def _state(eng):
    return kit.snapshot(eng, BUFFERS)


def _ingest(eng, rows):
    eng.ingest(*[torch.from_numpy(np.ascontiguousarray(x)) for x in rows])


NO_TREE = torch.empty(0, dtype=torch.float64)


def _inject(eng, rows, max_priority=1.0):
    size = len(rows[2])
    eng.ext.load_replay_state(eng.h, *[torch.from_numpy(x) for x in rows],
                              NO_TREE, NO_TREE, size, size, max_priority)


def _replay(eng):
    st = eng.ext.replay_state(eng.h)
    out = {k: st[k].numpy() for k in ("s", "a", "s2", "sum_tree", "min_tree")}
    out["r"], out["d"] = st["r"].numpy().ravel(), st["d"].numpy().ravel()
    out["size"], out["pos"] = int(st["size"]), int(st["pos"])
    return out


def _trained(B, mods, tr, **kw):
    return kit.engine(_shape(B), mods, tr, capacity=N, **kw)


# ---------------------------------------------------------------------------
# 1. the draw, exactly
# ---------------------------------------------------------------------------

# p_sample (B=64) and k_per_sample on the row-block (300) and wide (640) paths
@pytest.mark.parametrize("capacity,size", [(512, 300), (1024, 700)])
@pytest.mark.parametrize("B", [64, 300, 640])
def test_exact_draw(B, capacity, size):
    eng = _engine(B, capacity)
    eng.load_from_modules(*_modules())
    rows = _rows(np.random.default_rng(capacity), size)
    _inject(eng, rows)
    s, a, r, s2, d = rows
    for steps_done in (0, 5, 50):
        eng.set_schedule(steps_done)
        cnt = eng.counters()
        assert cnt["rng_epoch"] == steps_done and cnt["size"] == size
        eng.step(1)
        want = uniform_batch(SEED, steps_done + 1, B, size)
        idx = eng.read("bidx").numpy()
        assert np.array_equal(idx, want)
        assert idx.max() < size and len(np.unique(idx)) > 8
        assert np.array_equal(eng.read("bw").numpy(), np.ones(B, np.float32))
        assert np.array_equal(eng.read("br").numpy(), r[idx])
        assert np.array_equal(eng.read("bd").numpy(), d[idx])
        assert np.array_equal(eng.read("ba").numpy(), a[idx])
        assert np.array_equal(eng.read("bs2").numpy(), s2[idx])
        assert np.array_equal(eng.read("bs").numpy(), s[idx])


# ---------------------------------------------------------------------------
# 2. multi-step determinism, bitwise
# ---------------------------------------------------------------------------

# B = 48, 64: tail-crew pre-sample; 80: under the actor Adam; 128: re-sample
@pytest.mark.parametrize("B", [48, 64, 80, 128])
def test_multistep_launch_matches_single_steps(B):
    mods, tr = _modules(seed=B), _transitions(seed=B)
    x, y, z = (_trained(B, mods, tr) for _ in range(3))
    assert x._persistent and not x.info()["prioritized"]
    x.step(5)
    kit.assert_bs_is_gathered(x, "step(5)")
    epochs = []
    for i in range(5):
        y.step(1)
        kit.assert_bs_is_gathered(y, f"step(1) #{i + 1}")
        epochs.append(y.read("bidx").numpy())
    # every step drew with its own epoch (a pre-sample one epoch off shows
    # here as well as in the comparison below)
    for i, idx in enumerate(epochs):
        assert np.array_equal(idx, uniform_batch(13, i + 1, B, N))
    ref = _state(y)
    kit.assert_bitwise(_state(x), ref, "step(5) vs 5 x step(1)")
    z.step(2)
    z.step(3)
    kit.assert_bs_is_gathered(z, "step(2)+step(3)")
    kit.assert_bitwise(_state(z), ref, "step(2)+step(3) vs 5 x step(1)")
    assert np.array_equal(x.read("bidx").numpy(),
                          uniform_batch(13, 5, B, N))
    assert ref[0]["cnt:rng_epoch"] == ref[0]["cnt:beta_t"] == 5


def test_graph_replay_matches_uncaptured_rowblock():
    B = 300
    mods, tr = _modules(seed=B), _transitions(seed=B)
    x, y = _trained(B, mods, tr), _trained(B, mods, tr)
    assert not x._persistent
    x.step(6)
    y.train_steps(6, steps_per_graph=3)
    assert y._captured == 3
    kit.assert_bitwise(_state(x), _state(y), "step(6) vs graph 2 x 3")
    assert x.counters()["adam_t_critic"] == 6
    assert np.array_equal(x.read("bidx").numpy(),
                          uniform_batch(13, 6, B, N))


# ---------------------------------------------------------------------------
# 3. one step against eager torch
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("B", [64, 300, 640])
def test_step_parity_with_eager(B):
    mods, tr = _modules(seed=B), _transitions(seed=B)
    eng = _trained(B, mods, tr)
    eng.step(1)
    idx = eng.read("bidx").numpy()
    assert np.array_equal(idx, uniform_batch(13, 1, B, N))
    eager = kit.Eager(mods, LR, TAU, head=kit.CategoricalHead(
        V_MIN, V_MAX, GAMMA_N, K))
    eager.step(*[t[idx] for t in tr])
    # test_gpu_multistep.py's tolerances: the wide path's gradient bounds
    # (1e-4 absolute, 1e-3 of the slab's largest entry) and 6e-5 on the
    # parameter, target and moment slabs (1e-4 of the largest entry on the
    # moments)
    for n, want in eager.grads().items():
        got = eng.store_slab(n).numpy()
        print(f"B={B} {n}: max abs err {np.abs(got - want).max():.3g} "
              f"(max |ref| {np.abs(want).max():.3g})")
        np.testing.assert_allclose(got, want, atol=1e-4, err_msg=n)
        assert np.abs(got - want).max() <= 1e-3 * np.abs(want).max(), n
    slabs = eager.slabs()
    for n, want in slabs.items():
        got = eng.store_slab(n).numpy()
        print(f"B={B} {n}: max abs err {np.abs(got - want).max():.3g} "
              f"(max |ref| {np.abs(want).max():.3g})")
        np.testing.assert_allclose(got, want, atol=6e-5, err_msg=n)
    for n in ("m_actor", "m_critic", "v_actor", "v_critic"):
        got = eng.store_slab(n).numpy()
        assert np.abs(got - slabs[n]).max() <= 1e-4 * np.abs(slabs[n]).max(), n


@pytest.mark.parametrize("B", [64, 300, 640])
def test_is_weighting_is_a_no_op(B):
    mods, tr = _modules(seed=B), _transitions(seed=B)
    out = []
    for flag in (True, False):
        eng = _trained(B, mods, tr, is_weighting=flag)
        eng.step(2)
        assert np.array_equal(eng.read("bw").numpy(), np.ones(B, np.float32))
        out.append(_state(eng))
    kit.assert_bitwise(out[0], out[1], "is_weighting True vs False")


# ---------------------------------------------------------------------------
# 4. no trees
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("B", [64, 300, 640])
def test_no_trees(B):
    mods, tr = _modules(), _transitions()
    eng = _trained(B, mods, tr)
    info = eng.info()
    assert info["tree_cap"] == 0 and info["prioritized"] is False
    eng.set_schedule(0, max_priority=0.25)
    eng.step(3)
    _ingest(eng, _rows(np.random.default_rng(1), 10))
    assert eng.counters()["max_priority"] == 0.25
    st = eng.ext.replay_state(eng.h)
    assert st["sum_tree"].numel() == 0 and st["min_tree"].numel() == 0
    assert st["sum_tree"].dtype == torch.float64
    assert eng.read("sum_tree").numel() == 0
    assert eng.read("min_tree").numel() == 0
    # the priorities are still computed (and ignored)
    assert (eng.read("pri").numpy() > 0).all()
    # a PER engine of the same shape does keep them
    assert _engine(B, N, prioritized=True).info()["tree_cap"] == N


# ---------------------------------------------------------------------------
# 5. the write side against the plain numpy ring
# ---------------------------------------------------------------------------

def _check_ring(eng, ring):
    st = _replay(eng)
    assert (st["size"], st["pos"]) == (ring.size, ring.pos)
    for name, want in zip(("s", "a", "r", "s2", "d"), ring.occupied()):
        assert np.array_equal(st[name], want), name
    assert st["sum_tree"].size == 0 and st["min_tree"].size == 0
    return st


def _same_rows(x, y):
    return all(np.array_equal(x[k], y[k])
               for k in ("s", "a", "r", "s2", "d", "size", "pos"))


# one-workgroup path across the ring's end (capacity 600); the 4096 | 4097
# path switch and the bulk path across the ring's end (capacity 5000)
@pytest.mark.parametrize("capacity,calls", [
    (600, [300, 250, 50, 1, 100, 599]),
    (5000, [4096, 4097, 4097]),
])
def test_ingest_matches_ring(capacity, calls):
    eng = _engine(64, capacity)
    per = _engine(64, capacity, prioritized=True)
    ring = orc.RingOracle(capacity, per.info()["tree_cap"])
    rng = np.random.default_rng(capacity)
    for T in calls:
        rows = _rows(rng, T)
        _ingest(eng, rows)
        _ingest(per, rows)
        ring.add(*rows)
        st = _check_ring(eng, ring)
    assert ring.pos == sum(calls) % capacity and ring.size == capacity
    assert _same_rows(st, _replay(per))
    assert eng.counters()["max_priority"] == 1.0


def test_synth_fill_rows_equal_per_engine():
    u, p = _engine(64, 1000), _engine(64, 1000, prioritized=True)
    u.synth_fill(777, seed=5)
    p.synth_fill(777, seed=5)
    su, sp = _replay(u), _replay(p)
    assert (su["size"], su["pos"]) == (777, 777)
    assert _same_rows(su, sp)
    assert su["sum_tree"].size == 0 and sp["sum_tree"].size == 2048


def test_pendulum_rollout_episode():
    M, N, HOR = 8, 2, 4
    cap = M * (HOR - N + 1)
    rng = np.random.default_rng(11)
    th0 = rng.uniform(-np.pi, np.pi, M).astype(np.float32)
    td0 = rng.uniform(-1, 1, M).astype(np.float32)
    states = {}
    for prioritized in (True, False):
        # test_gpu_rollout.py's engine: one seed for the engine and the nets
        eng, net = kit.producer_engine(
            3, 1, hidden=256, n_atoms=51, capacity=cap, seed=4, v_min=-300.0,
            v_max=0.0, gamma_n=0.99 ** 5, lr=1e-4, prioritized=prioritized,
            actor_seed=4, critic_seed=None)
        eng.rollout_alloc(M, N, horizon=HOR, gamma=0.99, eps=0.0, seed=9)
        eng.rollout_set_state(th0, td0)
        env_steps, emitted = eng.rollout_run(1, reset=False, use_graph=False)
        assert env_steps == M * HOR and emitted == cap
        states[prioritized] = _replay(eng)
    st = states[False]                      # eng is the uniform engine now
    assert (st["size"], st["pos"]) == (cap, 0)
    assert st["sum_tree"].size == 0 and states[True]["sum_tree"].size > 0
    assert _same_rows(st, states[True])
    assert eng.counters()["max_priority"] == 1.0
    # against the host twins, at test_gpu_rollout.py's tolerances
    s, a, r, s2, d = eng.replay_rows()
    S, Aa, R, S2, D = orc.cpu_rollout(net, th0, td0, M, N, HOR)
    assert s.shape == S.shape
    np.testing.assert_allclose(a, Aa, rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(s, S, rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(s2, S2, rtol=2e-4, atol=3e-3)
    np.testing.assert_allclose(r, R, rtol=2e-3, atol=5e-3)
    assert np.array_equal(d, D)
    assert d[-M:].sum() == M and d[:-M].sum() == 0
    # a second, reset episode through the captured graph still has no sweep
    eng.rollout_run(1, reset=True, use_graph=True)
    assert eng.counters()["size"] == cap and eng.counters()["pos"] == 0


def test_goal_rollout_episode():
    n, ratio = 1, 0.8
    assert (go.M, go.HOR) == (8, 10)
    pos0, goal0 = go.starts()
    states = {}
    for prioritized in (False, True):
        eng = go.make_engine(go.episode_max(go.M, n, go.HOR),
                             seed=go.NET_SEED, prioritized=prioritized)
        eng.goal_rollout_alloc(go.M, n, horizon=go.HOR, gamma=go.GAMMA,
                               speed=go.SPEED, tol=go.TOL, her_ratio=ratio,
                               eps=go.EPS, seed=go.SEED)
        eng.goal_rollout_set_state(pos0, goal0)
        env_steps, rows, successes = eng.goal_rollout_run(
            1, reset=False, use_graph=False)
        states[prioritized] = _replay(eng)
        if prioritized:
            continue
        epi = go.device_episode(eng)
        go.assert_margin(epi["ep_pos"], epi["len"], epi["goal"], ratio)
        want = go.oracle_rows(epi, n, ratio)
        got = eng.rollout_last_rows()
        go.assert_rows_equal(got, want, n)
        assert rows == len(want[2]) > epi["len"].sum()      # some HER rows
        st = states[False]
        assert (st["size"], st["pos"]) == (
            rows, rows % go.episode_max(go.M, n, go.HOR))
        for k, w in zip(("s", "a", "r", "s2", "d"), got):
            assert np.array_equal(st[k], w), k
        assert st["sum_tree"].size == 0
        assert eng.counters()["max_priority"] == 1.0
    assert _same_rows(states[False], states[True])


# ---------------------------------------------------------------------------
# 6. resume
# ---------------------------------------------------------------------------

def _agent(seed=0, prioritized=False, **kw):
    return kit.agent(memory_size=8192, prioritized=prioritized, seed=seed,
                     **kw)


_fill = kit.fill_agent
_flat_params = kit.flat_params


def test_resume_bitwise_and_cross_mode_refusal():
    a1 = _agent(seed=0)
    _fill(a1, 2000)
    for _ in range(3):
        a1.train()
    st = a1.state_dict()
    assert st["engine"]["prioritized"] is False
    assert st["engine"]["counters"]["adam_t_actor"] == 3
    assert int(st["replay"]["size"]) == 2000
    assert st["replay"]["sum_tree"].numel() == 0
    for _ in range(2):
        a1.train()
    ref = _flat_params(a1)

    a2 = _agent(seed=99)
    _fill(a2, 50, seed=1)           # different replay: must be overwritten
    a2.load_state_dict(copy.deepcopy(st))
    eng2 = a2.engine.engine
    assert not eng2.info()["prioritized"]
    cnt = eng2.counters()
    assert cnt["adam_t_actor"] == cnt["rng_epoch"] == 3 and cnt["size"] == 2000
    for _ in range(2):
        a2.train()
    assert np.array_equal(_flat_params(a2), ref)
    e1 = a1.engine.engine
    for n in ("m_actor", "v_actor", "m_critic", "v_critic"):
        assert np.array_equal(e1.store_slab(n).numpy(),
                              eng2.store_slab(n).numpy()), n
    assert np.array_equal(e1.read("bidx").numpy(), eng2.read("bidx").numpy())

    # no conversion between the modes, in either direction
    per = _agent(seed=1, prioritized=True)
    with pytest.raises(ValueError, match="replay mode"):
        per.load_state_dict(copy.deepcopy(st))
    _fill(per, 200)
    per.train()
    st_per = per.state_dict()
    assert st_per["engine"]["prioritized"] is True
    with pytest.raises(ValueError, match="replay mode"):
        _agent(seed=2).load_state_dict(st_per)
    # and below the agent: the engine refuses a snapshot with trees
    rp = st_per["replay"]
    with pytest.raises(RuntimeError, match="tree size mismatch"):
        eng2.ext.load_replay_state(
            eng2.h, rp["s"], rp["a"], rp["r"], rp["s2"], rp["d"],
            rp["sum_tree"], rp["min_tree"], int(rp["size"]), int(rp["pos"]),
            1.0)
    with pytest.raises(ValueError, match="replay mode"):
        a2.replayBuffer.load_state_dict(rp)
    # params and optimizer state alone do cross
    _agent(seed=3).load_state_dict(st_per, load_replay=False)


# ---------------------------------------------------------------------------
# 7. wiring
# ---------------------------------------------------------------------------

def test_ddpg_forwards_the_replay_options():
    a = _agent(seed=5, true_td_priorities=True)
    from d4pg_amd.replay.uniform import Replay
    assert isinstance(a.replayBuffer, Replay)
    _fill(a, 100)
    a.train()
    info = a.engine.engine.info()
    assert info["prioritized"] is False and info["true_td"] is True
    assert info["tree_cap"] == 0
    cnt = a.engine.engine.counters()
    assert cnt["size"] == 100 and cnt["adam_t_actor"] == 1
    b = _agent(seed=5, prioritized=True)
    _fill(b, 100)
    b.train()
    info = b.engine.engine.info()
    assert info["prioritized"] is True and info["true_td"] is False
    assert info["tree_cap"] == 8192
