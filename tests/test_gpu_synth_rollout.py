"""Device synthetic-spec rollout (ops/hip/engine_synth.hip), any (obs, act),
against its host twin: VectorSynthetic + VecNStep driven by the torch actor
and the philox noise oracles (_synth_oracles.py).

Tolerances.  Every compared value is bounded by 1 in magnitude (tanh states,
clipped actions, rewards in [-1, 0.1]), so rows are held to the project's
unit-scale bound, atol 2e-4 (the a / s bound of test_gpu_rollout_exact.py).
The bound does not cover for rounding: each parity test first measures the
float32 twin against a float64 run of the same recurrence on its own inputs
and asserts that deviation is below 5e-5.  Streams are read value by value at
atol 5e-5 (1e-6 for the reset state): float32 logf/cosf/tanhf against the
oracle's float64.
"""

import functools

import numpy as np
import pytest
import torch

import _engine_kit as kit
import _oracles as orc
import _synth_oracles as so
from d4pg_amd.envs.vector import PhiloxProcNoise, VecNStep, VectorSynthetic

pytestmark = pytest.mark.gpu

H, K = 64, 51
GAMMA = 0.99
DIST = {"type": "categorical", "v_min": -10.0, "v_max": 1.0, "n_atoms": K}
SEED = 77                               # rollout seed (reset, noise streams)
ENV_SEED = 5                            # names W, U
NET_SEED = 4
ALPHA = np.float64(np.float32(0.6))     # the engine holds per_alpha as float
ATOL = 2e-4
TWIN_F64_BOUND = 5e-5


@functools.lru_cache(maxsize=None)
def _net(o, a, hidden=H):
    """Actor with its head scaled up from the 3e-3 init, so that actions
    spread over (-1, 1) instead of sitting at 0."""
    return kit.producer_nets(o, a, DIST, hidden=hidden, actor_seed=NET_SEED,
                             critic_seed=NET_SEED, head_gain=60.0)[0]


def make_engine(o, a, capacity, prioritized=True, hidden=H, batch=64):
    return kit.producer_engine(
        o, a, hidden=hidden, n_atoms=K, capacity=capacity, batch=batch,
        seed=0, v_min=-10.0, v_max=1.0, gamma_n=GAMMA ** 3, lr=1e-4,
        prioritized=prioritized, actor_seed=NET_SEED, critic_seed=NET_SEED,
        head_gain=60.0)[0]


def _twin(o, a, m, hor, act_high=1.0, proc_sigma=0.0, ep=1):
    return VectorSynthetic(m, o, a, horizon=hor, act_high=act_high,
                           seed=ENV_SEED, proc_sigma=proc_sigma,
                           proc_noise=PhiloxProcNoise(SEED, ep))


def _state0(o, m, seed=3):
    return np.clip(0.5 * np.random.default_rng(seed).standard_normal((m, o)),
                   -1.0, 1.0).astype(np.float32)


def _state(eng):
    st = eng.ext.replay_state(eng.h)
    out = {k: st[k].numpy() for k in ("s", "a", "s2", "sum_tree", "min_tree")}
    for k in ("r", "d"):
        out[k] = st[k].numpy().ravel()
    out["size"], out["pos"] = int(st["size"]), int(st["pos"])
    out["max_priority"] = float(st["max_priority"])
    return out


def _oracle(o, a, m, n, hor, state0, act_high=1.0, eps=0.0, proc_sigma=0.0,
            ep=1, kind="gaussian", **ou):
    """Twin rows for one episode from `state0`, after checking the twin's
    own float32 rounding against the float64 recurrence."""
    vec = _twin(o, a, m, hor, act_high, proc_sigma, ep)
    mk = lambda: so.Exploration(m, a, SEED, ep, kind=kind, eps=eps, **ou)
    rows, acts = so.twin_episode(_net(o, a), vec, VecNStep(m, o, a, n, GAMMA),
                                 state0, mk())
    rows64 = so.f64_episode(_net(o, a), vec.W, vec.U, state0, mk(), n=n,
                            horizon=hor, gamma=GAMMA, act_high=act_high,
                            proc_sigma=proc_sigma, proc_seed=SEED, ep=ep)
    dev = so.max_dev(rows, rows64)
    print(f"({o}, {a}) M={m} n={n} hor={hor}: twin f32 vs f64 {dev:.3g}")
    assert dev < TWIN_F64_BOUND, "misconfigured test: shorten the horizon"
    assert np.array_equal(rows[4], rows64[4])
    return vec, rows, acts


def assert_rows_close(got, want, tag=""):
    assert len(got[2]) == len(want[2])
    errs = {k: float(np.abs(g.astype(np.float64) - w).max())
            for k, g, w in zip(("s", "a", "r", "s2"), got, want)}
    print(f"{tag} max abs err " + " ".join(f"{k} {v:.3g}"
                                           for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= ATOL, (k, v)
    assert np.array_equal(got[4], want[4])
    return errs


def _run_injected(o, a, m, n, hor, state0, act_high=1.0, capacity=None,
                  **alloc):
    vec = _twin(o, a, m, hor, act_high)
    eng = make_engine(o, a, capacity or m * (hor - n + 1))
    alloc.setdefault("eps", 0.0)
    alloc.setdefault("proc_sigma", 0.0)
    eng.synth_rollout_alloc(m, n, vec.W, vec.U, horizon=hor, gamma=GAMMA,
                            act_high=act_high, seed=SEED, **alloc)
    eng.synth_rollout_set_state(state0)
    out = eng.synth_rollout_run(1, reset=False, use_graph=False)
    return eng, out


# ---------------------------------------------------------------------------
# single tick and short episodes from an injected state
# ---------------------------------------------------------------------------

SHAPES = [(5, 2, 8, 1.0, [(1, 4), (3, 10), (4, 4)]),
          (70, 3, 8, 1.0, [(1, 4), (3, 10), (4, 4)]),
          (376, 17, 8, 0.4, [(1, 3), (3, 3)])]
CASES = [(o, a, m, hi, n, hor) for o, a, m, hi, nh in SHAPES
         for n, hor in nh]


@pytest.mark.parametrize("o,a,m,act_high,n,hor", CASES)
def test_injected_episode_parity(o, a, m, act_high, n, hor):
    state0 = _state0(o, m)
    _, want, acts = _oracle(o, a, m, n, hor, state0, act_high)
    # the actions the mutations hinge on are not degenerate
    assert np.abs(acts).mean() > 0.05 and np.abs(acts).max() < 1.0
    eng, (env_steps, emitted) = _run_injected(o, a, m, n, hor, state0,
                                              act_high)
    count = m * (hor - n + 1)
    assert (env_steps, emitted) == (m * hor, count)
    assert_rows_close(eng.rollout_last_rows(), want, f"({o}, {a}) n={n}")
    st = _state(eng)
    assert (st["size"], st["pos"]) == (count, 0)    # capacity == one episode
    info = eng.synth_rollout_info()
    assert (info["base"], info["episode"], info["O"], info["A"]) == \
        (0, 1, o, a)
    # slot placement: row emit_k * M + i sits in slot emit_k * M + i
    for k, w in zip(("s", "a", "r", "s2", "d"), eng.rollout_last_rows()):
        assert np.array_equal(st[k], w), k
    assert (st["d"][:-m] == 0).all() and (st["d"][-m:] == 1).all()
    # ra holds the normalized action, not the env-scaled one
    np.testing.assert_allclose(st["a"][:m], acts[0], rtol=0, atol=ATOL)


def test_injected_episode_parity_with_both_noises():
    """Process noise on top of non-zero W, U, with exploration noise on:
    the streams and the dynamics together, against the float32 twin and
    against the float64 recurrence written out in the oracle file (which
    does not go through the library's philox source)."""
    o, a, m, n, hor, act_high, eps, sigma = 17, 6, 8, 3, 6, 0.4, 0.3, 0.01
    state0 = _state0(o, m)
    vec, want, acts = _oracle(o, a, m, n, hor, state0, act_high, eps=eps,
                              proc_sigma=sigma)
    assert (np.abs(acts) < 1.0).mean() >= 0.75
    eng, (_, emitted) = _run_injected(o, a, m, n, hor, state0, act_high,
                                      eps=eps, proc_sigma=sigma)
    assert emitted == m * (hor - n + 1)
    rows = eng.rollout_last_rows()
    assert_rows_close(rows, want, "both noises, twin")
    want64 = so.f64_episode(
        _net(o, a), vec.W, vec.U, state0,
        so.Exploration(m, a, SEED, 1, eps=eps), n=n, horizon=hor,
        gamma=GAMMA, act_high=act_high, proc_sigma=sigma, proc_seed=SEED)
    assert_rows_close(rows, want64, "both noises, float64")
    # the noise is in the rows: the noiseless episode is far from them
    _, quiet, _ = _oracle(o, a, m, n, hor, state0, act_high)
    assert np.abs(rows[3] - quiet[3]).max() > 100 * ATOL


# ---------------------------------------------------------------------------
# the MFMA forward path (policy chain and mixing GEMM from 512 rows up)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("m", [512, 520])
def test_mfma_forward_path(m):
    o, a, n, hor = 17, 6, 2, 4
    state0 = _state0(o, m)
    _, want, _ = _oracle(o, a, m, n, hor, state0)
    eng, (_, emitted) = _run_injected(o, a, m, n, hor, state0)
    assert emitted == m * (hor - n + 1)
    assert_rows_close(eng.rollout_last_rows(), want, f"M={m}")
    st = _state(eng)
    assert (st["size"], st["pos"]) == (emitted, 0)


# ---------------------------------------------------------------------------
# the philox streams, value by value, at M = 64
# ---------------------------------------------------------------------------

def test_reset_stream_exact():
    o, a, m = 5, 3, 64
    vec = _twin(o, a, m, 1)
    eng = make_engine(o, a, m)
    eng.synth_rollout_alloc(m, 1, vec.W, vec.U, horizon=1, eps=0.0,
                            proc_sigma=0.0, seed=SEED)
    eng.synth_rollout_run(1, reset=True, use_graph=False)
    s = eng.rollout_last_rows()[0]
    want = so.reset_state(SEED, 1, m, o)
    print(f"reset state: max abs err {np.abs(s - want).max():.3g}")
    np.testing.assert_allclose(s, want, rtol=0, atol=1e-6)
    assert len(np.unique(want)) == m * o and np.abs(want).max() < 0.6


def _noise_from_rows(o, a, rows):
    """Stored action minus the policy's output at the stored state."""
    with torch.no_grad():
        mu = _net(o, a)(torch.from_numpy(rows[0])).numpy()
    return rows[1].astype(np.float64) - mu


def test_gaussian_action_stream_exact():
    o, a, m, hor, eps = 5, 3, 64, 3, 0.3
    state0 = _state0(o, m)
    _, want, acts = _oracle(o, a, m, 1, hor, state0, eps=eps)
    inner = np.abs(acts) < 1.0 - 1e-3              # from the oracle alone
    assert inner[:, :, [0, a - 1]].mean() >= 0.75
    eng, _ = _run_injected(o, a, m, 1, hor, state0, eps=eps)
    rows = eng.rollout_last_rows()
    got = _noise_from_rows(o, a, rows).reshape(hor, m, a)
    for t in range(hor):
        noise = eps * so.act_normals(SEED, 1, t, m, a)
        assert np.abs(noise[:, 0] - noise[:, a - 1]).min() > 0
        for k in (0, a - 1):
            ok = inner[t, :, k]
            err = np.abs(got[t, ok, k] - noise[ok, k]).max()
            print(f"tick {t} dim {k}: {ok.sum()} unclipped, err {err:.3g}")
            assert err <= 5e-5
    assert_rows_close(rows, want, "gaussian")


@pytest.mark.parametrize("mu", [0.0, 0.25])
def test_ou_stream_exact(mu):
    o, a, m, hor, eps = 5, 3, 64, 6, 1.0
    state0 = _state0(o, m)
    ou = dict(ou_theta=0.15, ou_sigma=0.2, ou_mu=mu)
    _, want, acts = _oracle(o, a, m, 1, hor, state0, eps=eps, kind="ou", **ou)
    inner = np.abs(acts) < 1.0 - 1e-3
    assert inner[:, :, [0, a - 1]].mean() >= 0.75
    eng, _ = _run_injected(o, a, m, 1, hor, state0, eps=eps, noise="ou", **ou)
    rows = eng.rollout_last_rows()
    got = _noise_from_rows(o, a, rows).reshape(hor, m, a)
    ex = so.Exploration(m, a, SEED, 1, kind="ou", eps=eps, **ou)
    for t in range(hor):
        x = ex(t)
        for k in (0, a - 1):
            ok = inner[t, :, k]
            err = np.abs(got[t, ok, k] - x[ok, k]).max()
            print(f"mu {mu} tick {t} dim {k}: {ok.sum()} unclipped, "
                  f"err {err:.3g}")
            assert err <= 5e-5
    assert abs(ex.x.mean() - mu) < 0.02 and ex.x.std() > 0.02
    assert_rows_close(rows, want, f"ou mu={mu}")


def test_process_noise_stream_exact():
    """W = U = 0 and sigma = 0.5: s2 = tanh(0.5 * n01) reads the draw off."""
    o, a, m, hor = 5, 3, 64, 2
    eng = make_engine(o, a, m * hor)
    eng.synth_rollout_alloc(m, 1, np.zeros((o, o)), np.zeros((a, o)),
                            horizon=hor, eps=0.0, proc_sigma=0.5, seed=SEED)
    eng.synth_rollout_set_state(_state0(o, m))
    eng.synth_rollout_run(1, reset=False, use_graph=False)
    s2 = eng.rollout_last_rows()[3].reshape(hor, m, o)
    for t in range(hor):
        g = so.proc_normals(SEED, 1, t, m, o)
        assert np.abs(g[:, 0] - g[:, o - 1]).min() > 0
        for k in (0, o - 1):
            err = np.abs(s2[t, :, k] - np.tanh(0.5 * g[:, k])).max()
            print(f"tick {t} dim {k}: err {err:.3g}")
            assert err <= 5e-5


# ---------------------------------------------------------------------------
# ring wrap, leaves and the per-episode tree rebuild
# ---------------------------------------------------------------------------

def test_ring_wrap_and_trees():
    o, a, m, n, hor, cap = 5, 2, 8, 3, 10, 100
    per_ep = m * (hor - n + 1)
    assert per_ep == 64 and cap % per_ep != 0
    s_a, s_b = _state0(o, m, seed=1), _state0(o, m, seed=2)
    eng, _ = _run_injected(o, a, m, n, hor, s_a, capacity=cap)
    tree_cap = eng.info()["tree_cap"]
    assert tree_cap == 128                  # > capacity
    ep1 = _state(eng)
    assert (ep1["size"], ep1["pos"]) == (per_ep, per_ep)
    want_s, want_m = orc.build_trees(np.ones(per_ep), tree_cap)
    assert np.array_equal(ep1["sum_tree"], want_s)
    assert np.array_equal(ep1["min_tree"], want_m)

    eng.set_schedule(0, max_priority=2.5)
    eng.synth_rollout_set_state(s_b)
    eng.synth_rollout_run(1, reset=False, use_graph=False)
    st = _state(eng)
    assert (st["size"], st["pos"]) == (cap, 2 * per_ep - cap)
    info = eng.synth_rollout_info()
    assert (info["base"], info["episode"]) == (per_ep, 2)
    slots = (per_ep + np.arange(per_ep)) % cap
    _, want, _ = _oracle(o, a, m, n, hor, s_b, ep=2)
    assert_rows_close(tuple(st[k][slots] for k in ("s", "a", "r", "s2", "d")),
                      want, "episode 2")
    for g, w in zip(eng.rollout_last_rows(),
                    (st[k][slots] for k in ("s", "a", "r", "s2", "d"))):
        assert np.array_equal(g, w)
    kept = np.setdiff1d(np.arange(cap), slots)
    assert np.array_equal(kept, np.arange(2 * per_ep - cap, per_ep))
    for k in ("s", "a", "r", "s2", "d"):
        assert np.array_equal(st[k][kept], ep1[k][kept]), k

    leaves = st["sum_tree"][tree_cap:tree_cap + cap]
    assert (leaves[kept] == 1.0).all()
    new = np.float64(np.float32(2.5)) ** ALPHA
    ulps = np.abs(leaves[slots] - new) / np.spacing(new)
    print(f"2.5^alpha leaves: max {ulps.max():.0f} ulp from the host pow")
    assert (ulps <= 2).all()
    assert np.array_equal(st["min_tree"][tree_cap:tree_cap + cap], leaves)
    # past the capacity nothing was ever written
    assert (st["sum_tree"][tree_cap + cap:] == 0).all()
    assert np.isinf(st["min_tree"][tree_cap + cap:]).all()
    want_s, want_m = orc.build_trees(leaves, tree_cap)
    assert np.array_equal(st["sum_tree"], want_s)
    assert np.array_equal(st["min_tree"], want_m)


def test_untouched_slots_stay_empty():
    o, a, m, n, hor, cap = 5, 2, 8, 3, 10, 100
    eng, (_, emitted) = _run_injected(o, a, m, n, hor, _state0(o, m),
                                      capacity=cap)
    full = eng.ext.replay_slice(eng.h, 0, cap)
    for t in full:
        assert (t.numpy()[emitted:] == 0).all()


# ---------------------------------------------------------------------------
# graph replay == uncaptured launches; uniform replay
# ---------------------------------------------------------------------------

def _two_episodes(use_graph, prioritized=True):
    o, a, m, n, hor = 17, 6, 64, 3, 8
    vec = _twin(o, a, m, hor)
    eng = make_engine(o, a, 2 * m * (hor - n + 1) + 40,
                      prioritized=prioritized)
    eng.synth_rollout_alloc(m, n, vec.W, vec.U, horizon=hor, gamma=GAMMA,
                            eps=0.3, proc_sigma=0.01, seed=13)
    out = eng.synth_rollout_run(2, reset=True, use_graph=use_graph)
    assert out == (2 * m * hor, 2 * m * (hor - n + 1))
    return eng, _state(eng)


def test_graph_replay_equals_uncaptured_bitwise():
    (eg, sg), (eu, su) = _two_episodes(True), _two_episodes(False)
    rows = 2 * 64 * 6
    assert (sg["size"], sg["pos"]) == (rows, rows)
    assert eg.synth_rollout_info() == eu.synth_rollout_info()
    assert eg.synth_rollout_info()["episode"] == 2
    for k in sg:
        assert np.array_equal(sg[k], su[k]), k
    # the philox epoch advanced inside the graph: episode 2 is new data
    assert not np.array_equal(sg["s"][:64], sg["s"][rows // 2:rows // 2 + 64])
    tree_cap = eg.info()["tree_cap"]
    leaves = sg["sum_tree"][tree_cap:][:rows]
    assert (leaves == 1.0).all()
    want_s, want_m = orc.build_trees(leaves, tree_cap)
    assert np.array_equal(sg["sum_tree"], want_s)
    assert np.array_equal(sg["min_tree"], want_m)


def test_uniform_replay_rows_equal_per_rows():
    eu, su = _two_episodes(True, prioritized=False)
    _, sp = _two_episodes(True, prioritized=True)
    assert eu.info()["tree_cap"] == 0
    assert len(su["sum_tree"]) == 0 and len(su["min_tree"]) == 0
    for k in ("s", "a", "r", "s2", "d", "size", "pos"):
        assert np.array_equal(su[k], sp[k]), k
    assert su["max_priority"] == 1.0 == sp["max_priority"]


# ---------------------------------------------------------------------------
# refusals (host-side checks; nothing is launched)
# ---------------------------------------------------------------------------

def test_refusals():
    o, a, m, n, hor = 5, 2, 8, 3, 10
    vec = _twin(o, a, m, hor)
    eng = make_engine(o, a, m * (hor - n + 1) - 1)
    with pytest.raises(RuntimeError, match="synth_rollout_alloc first"):
        eng.synth_rollout_run(1)
    with pytest.raises(RuntimeError, match="capacity"):
        eng.synth_rollout_alloc(m, n, vec.W, vec.U, horizon=hor)
    with pytest.raises(RuntimeError, match="horizon < n_steps"):
        eng.synth_rollout_alloc(1, n, vec.W, vec.U, horizon=n - 1)
    with pytest.raises(RuntimeError, match="2\\^20"):
        eng.synth_rollout_alloc(1, n, vec.W, vec.U, horizon=2 ** 20 - 2)
    with pytest.raises(RuntimeError, match="W is not"):
        eng.synth_rollout_alloc(1, n, vec.W[:, :-1], vec.U, horizon=hor)
    with pytest.raises(RuntimeError, match="W is not"):
        eng.synth_rollout_alloc(1, n, vec.U, vec.U, horizon=hor)
    with pytest.raises(RuntimeError, match="U is not"):
        eng.synth_rollout_alloc(1, n, vec.W, vec.U.T, horizon=hor)
    eng.synth_rollout_alloc(m - 1, n, vec.W, vec.U, horizon=hor)   # fits
    with pytest.raises(RuntimeError, match="rollout_alloc first"):
        eng.rollout_run(1)
    with pytest.raises(RuntimeError, match="goal_rollout_alloc first"):
        eng.goal_rollout_run(1)
    pend = kit.engine(kit.Shape(64, H, 3, 1, K, v_min=-50.0), capacity=4096,
                      seed=0, gamma_n=GAMMA)
    pend.rollout_alloc(8, 3, horizon=10)
    with pytest.raises(RuntimeError, match="synth_rollout_alloc first"):
        pend.synth_rollout_run(1)


# ---------------------------------------------------------------------------
# one pool and one episode graph, handed from producer to producer
# ---------------------------------------------------------------------------

def _life_engine(o, like=None):
    """(o, 1) engine with an 11-atom critic; `like`: take its four slabs."""
    kw = dict(hidden=H, n_atoms=11, capacity=64, seed=0, v_min=-10.0,
              v_max=1.0, gamma_n=GAMMA ** 2, lr=1e-4)
    if like is None:
        eng, _ = kit.producer_engine(o, 1, actor_seed=NET_SEED,
                                     critic_seed=NET_SEED, head_gain=60.0,
                                     **kw)
    else:
        eng = kit.engine(kit.Shape(64, H, o, 1, 11, v_min=-10.0, v_max=1.0),
                         capacity=64, seed=0, gamma_n=GAMMA ** 2)
        for name in ("actor", "actor_target", "critic", "critic_target"):
            eng.load_slab(name, like.store_slab(name))
    return eng


@pytest.mark.parametrize("kind", ["pendulum", "goal"])
def test_pool_and_graph_across_kinds(kind):
    """kind -> synth -> kind on one engine, every episode graph-captured:
    each allocation frees the previous producer's pool and graph, so what an
    episode writes is bitwise what an engine that ran only that step writes
    (the captured run resets the envs from the seed, after the injected
    state).  Pendulum's third episode wraps the 64-slot ring; the goal
    rollout's row counts depend on the episodes."""
    o = 3 if kind == "pendulum" else 2
    m, n, hor = 5, 2, 6
    vec = _twin(o, 1, m, hor)
    x0 = np.linspace(-0.8, 0.8, m, dtype=np.float32)

    def own(eng, seed):
        if kind == "pendulum":
            eng.rollout_alloc(m, n, horizon=hor, gamma=GAMMA, seed=seed)
            eng.rollout_set_state(2 * x0, x0[::-1].copy())
            return eng.rollout_run(1, reset=True, use_graph=True)
        eng.goal_rollout_alloc(m, n, horizon=hor, gamma=GAMMA, tol=0.3,
                               seed=seed)
        eng.goal_rollout_set_state(x0[:, None], -x0[:, None])
        return eng.goal_rollout_run(1, reset=True, use_graph=True)

    def synth(eng):
        eng.synth_rollout_alloc(m, n, vec.W, vec.U, horizon=hor, gamma=GAMMA,
                                seed=SEED)
        return eng.synth_rollout_run(1, reset=True, use_graph=True)

    eng = _life_engine(o)
    own(eng, seed=21)
    first = eng.counters()["pos"]
    assert synth(eng) == (m * hor, m * (hor - n + 1))
    only_synth = _life_engine(o, like=eng)
    synth(only_synth)
    rows = eng.rollout_last_rows()
    assert len(rows[2]) == m * (hor - n + 1)
    assert eng.synth_rollout_info()["base"] == first > 0
    for g, w in zip(rows, only_synth.rollout_last_rows()):
        assert np.array_equal(g, w)
    with pytest.raises(RuntimeError, match="rollout_alloc first"):
        eng.rollout_run(1)
    with pytest.raises(RuntimeError, match="goal_rollout_alloc first"):
        eng.goal_rollout_run(1)

    before = eng.counters()["pos"]
    out = own(eng, seed=22)
    only_last = _life_engine(o, like=eng)
    assert own(only_last, seed=22) == out
    rows = eng.rollout_last_rows()
    assert len(rows[2]) == out[1] > 0
    if kind == "pendulum":                          # 50 + 25 rows: wraps
        assert before + out[1] > 64
    assert eng.counters()["pos"] == (before + out[1]) % 64
    for g, w in zip(rows, only_last.rollout_last_rows()):
        assert np.array_equal(g, w)
    with pytest.raises(RuntimeError, match="synth_rollout_alloc first"):
        eng.synth_rollout_run(1)


# ---------------------------------------------------------------------------
# the learner trains on what the rollout wrote
# ---------------------------------------------------------------------------

def test_train_after_rollout():
    o, a, m, n, hor = 17, 6, 64, 2, 4
    vec = _twin(o, a, m, hor)
    eng = make_engine(o, a, 1024)
    eng.synth_rollout_alloc(m, n, vec.W, vec.U, horizon=hor, gamma=GAMMA,
                            eps=0.3, seed=SEED)
    _, emitted = eng.synth_rollout_run(1)
    assert emitted == 192 and eng.counters()["size"] == 192
    before = eng.counters()
    eng.step(3)
    cnt = eng.counters()
    assert cnt["adam_t_actor"] == before["adam_t_actor"] + 3
    assert cnt["adam_t_critic"] == before["adam_t_critic"] + 3
    assert cnt["size"] == 192
    q = eng.read("q")
    assert torch.isfinite(q).all()
    assert np.isfinite(cnt["loss_critic"]) and np.isfinite(cnt["loss_actor"])
