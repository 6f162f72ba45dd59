"""Exact checks of the device rollout's emit path (k_roll_begin, k_roll_reset,
k_roll_tick, k_roll_end and the per-episode tree rebuild).

Continuous values (s, a, r, s2) are compared with the numpy oracle of
test_gpu_rollout.py at that file's tolerances.  Everything discrete is
compared for equality: which ring slot every emit lands in, the done flags,
size and pos, the leaves of untouched slots and both trees.  The philox
streams behind the reset state and the exploration noise are reproduced on
the CPU (tests/_oracles.py), so the noise of every env at every tick is
checked value by value, not by its moments.
"""

import numpy as np
import pytest
import torch

import _engine_kit as kit
import _oracles as orc
from _oracles import cpu_rollout

pytestmark = pytest.mark.gpu

ALPHA = np.float64(np.float32(0.6))     # the engine holds per_alpha as float


def make_engine(capacity, seed=0, batch=64):
    """(engine, actor) of test_gpu_rollout.py: one seed for the engine, the
    actor and, continuing the actor's stream, the critic."""
    return kit.producer_engine(
        3, 1, hidden=256, n_atoms=51, capacity=capacity, batch=batch,
        seed=seed, v_min=-300.0, v_max=0.0, gamma_n=0.99 ** 5, lr=1e-4,
        actor_seed=seed, critic_seed=None)


def _state(eng):
    st = eng.ext.replay_state(eng.h)
    out = {k: st[k].numpy() for k in ("s", "s2", "sum_tree", "min_tree")}
    for k in ("a", "r", "d"):
        out[k] = st[k].numpy().ravel()
    out["size"], out["pos"] = int(st["size"]), int(st["pos"])
    return out


def _start(M, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-np.pi, np.pi, M).astype(np.float32),
            rng.uniform(-1, 1, M).astype(np.float32))


def _assert_parity(st, want, slots=None):
    """Device rows (at `slots`, default the first len(want) rows) against
    the oracle's (S, A, R, S2, D) at test_gpu_rollout.py's tolerances; done
    flags exactly."""
    S, Aa, R, S2, D = want
    if slots is None:
        slots = np.arange(len(R))
    np.testing.assert_allclose(st["a"][slots], Aa.ravel(), rtol=2e-4,
                               atol=2e-4)
    np.testing.assert_allclose(st["s"][slots], S, rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(st["s2"][slots], S2, rtol=2e-4, atol=3e-3)
    np.testing.assert_allclose(st["r"][slots], R, rtol=2e-3, atol=5e-3)
    assert np.array_equal(st["d"][slots], D)
    return {"a": float(np.abs(st["a"][slots] - Aa.ravel()).max()),
            "s": float(np.abs(st["s"][slots] - S).max()),
            "s2": float(np.abs(st["s2"][slots] - S2).max()),
            "r": float(np.abs(st["r"][slots] - R).max())}


def _assert_tree_invariant(st, cap, n_leaves):
    """Both trees bitwise what build_trees gives over the device's leaves;
    leaves past n_leaves still hold the fresh-engine fill."""
    leaves = st["sum_tree"][cap:cap + n_leaves]
    assert np.array_equal(st["min_tree"][cap:cap + n_leaves], leaves)
    want_s, want_m = orc.build_trees(leaves, cap)
    assert np.array_equal(st["sum_tree"], want_s)
    assert np.array_equal(st["min_tree"], want_m)


# ---------------------------------------------------------------------------
# n-step fold edges
# ---------------------------------------------------------------------------

# n = 1: every tick emits.  n = horizon: one emit, and it is the done one.
@pytest.mark.parametrize("N,HOR", [(1, 4), (3, 10), (4, 4)])
def test_fold_edges(N, HOR):
    M = 8
    cap = M * (HOR - N + 1)
    eng, net = make_engine(capacity=cap, seed=4)
    eng.rollout_alloc(M, N, horizon=HOR, gamma=0.99, eps=0.0, seed=9)
    th0, td0 = _start(M, 11)
    eng.rollout_set_state(th0, td0)
    env_steps, emitted = eng.rollout_run(1, reset=False, use_graph=False)
    assert env_steps == M * HOR and emitted == cap
    st = _state(eng)
    assert (st["size"], st["pos"]) == (cap, 0)
    err = _assert_parity(st, cpu_rollout(net, th0, td0, M, N, HOR))
    print(f"N={N} HOR={HOR}: max abs err {err}")
    assert st["d"][-M:].sum() == M and st["d"][:-M].sum() == 0
    tree_cap = eng.info()["tree_cap"]
    want_s, want_m = orc.build_trees(np.ones(cap), tree_cap)
    assert np.array_equal(st["sum_tree"], want_s)
    assert np.array_equal(st["min_tree"], want_m)


# ---------------------------------------------------------------------------
# ring placement across the ring's end, leaves and the per-episode rebuild
# ---------------------------------------------------------------------------

def test_ring_placement_and_wrap():
    M, N, HOR, cap = 8, 3, 10, 100
    per_ep = M * (HOR - N + 1)
    assert per_ep == 64
    eng, net = make_engine(capacity=cap, seed=4)
    tree_cap = eng.info()["tree_cap"]
    assert tree_cap == 128                  # > capacity
    eng.rollout_alloc(M, N, horizon=HOR, gamma=0.99, eps=0.0, seed=9)

    th1, td1 = _start(M, 11)
    eng.rollout_set_state(th1, td1)
    eng.rollout_run(1, reset=False, use_graph=False)
    ep1 = _state(eng)
    assert (ep1["size"], ep1["pos"]) == (per_ep, per_ep)
    _assert_parity(ep1, cpu_rollout(net, th1, td1, M, N, HOR))
    want_s, want_m = orc.build_trees(np.ones(per_ep), tree_cap)
    assert np.array_equal(ep1["sum_tree"], want_s)
    assert np.array_equal(ep1["min_tree"], want_m)

    eng.set_schedule(0, max_priority=2.5)
    th2, td2 = _start(M, 12)
    eng.rollout_set_state(th2, td2)
    eng.rollout_run(1, reset=False, use_graph=False)
    st = _state(eng)
    assert (st["size"], st["pos"]) == (100, 28)
    # emit (k, i) of episode 2 is row k*M + i of the oracle's output
    slots = (per_ep + np.arange(per_ep)) % cap
    err = _assert_parity(st, cpu_rollout(net, th2, td2, M, N, HOR), slots)
    print(f"episode 2 across the wrap: max abs err {err}")
    kept = np.setdiff1d(np.arange(cap), slots)
    assert np.array_equal(kept, np.arange(28, 64))
    for k in ("s", "a", "r", "s2", "d"):
        assert np.array_equal(st[k][kept], ep1[k][kept]), k
    # the two episodes are different data, so a misplaced row cannot pass
    assert np.abs(st["s"][:28] - ep1["s"][:28]).max() > 0.1

    leaves = st["sum_tree"][tree_cap:tree_cap + cap]
    assert (leaves[kept] == 1.0).all()
    want = np.float64(np.float32(2.5)) ** ALPHA
    ulps = np.abs(leaves[slots] - want) / np.spacing(want)
    print(f"2.5^alpha leaves: max {ulps.max():.0f} ulp from the host pow")
    assert (ulps <= 2).all()
    _assert_tree_invariant(st, tree_cap, cap)


# ---------------------------------------------------------------------------
# graph replay == uncaptured launches
# ---------------------------------------------------------------------------

def test_graph_replay_equals_uncaptured_bitwise():
    M, N, HOR = 64, 3, 8
    per_ep = M * (HOR - N + 1)
    states = []
    for use_graph in (True, False):
        eng, _ = make_engine(capacity=1024, seed=6)
        eng.rollout_alloc(M, N, horizon=HOR, eps=0.3, seed=13)
        eng.rollout_run(2, reset=True, use_graph=use_graph)
        states.append(_state(eng))
    g, u = states
    assert (g["size"], g["pos"]) == (2 * per_ep, 2 * per_ep)
    for k in g:
        assert np.array_equal(g[k], u[k]), k
    # the philox epoch advanced inside the graph: episode 2 is new data
    e1, e2 = g["s"][:per_ep], g["s"][per_ep:]
    assert np.abs(e1[:M] - e2[:M]).max() > 0.1
    assert not np.array_equal(g["a"][:per_ep], g["a"][per_ep:])
    _assert_tree_invariant(g, eng.info()["tree_cap"], 2 * per_ep)


# ---------------------------------------------------------------------------
# the MFMA policy forward (M >= 512), and M no multiple of 256 or of 64
# ---------------------------------------------------------------------------

# 520 rows: three k_roll_tick workgroups with a tail of 8, and a partial
# 64-row MFMA tile.  512 is the first M on the MFMA forward.
@pytest.mark.parametrize("M", [512, 520])
def test_mfma_forward_and_ragged_m(M):
    N, HOR = 2, 4
    cap = M * (HOR - N + 1)
    eng, net = make_engine(capacity=cap, seed=4)
    eng.rollout_alloc(M, N, horizon=HOR, gamma=0.99, eps=0.0, seed=9)
    th0, td0 = _start(M, 17)
    eng.rollout_set_state(th0, td0)
    eng.rollout_run(1, reset=False, use_graph=False)
    st = _state(eng)
    assert (st["size"], st["pos"]) == (cap, 0)
    err = _assert_parity(st, cpu_rollout(net, th0, td0, M, N, HOR))
    print(f"M={M}: max abs err {err}")
    assert st["d"][-M:].sum() == M and st["d"][:-M].sum() == 0
    tree_cap = eng.info()["tree_cap"]
    want_s, want_m = orc.build_trees(np.ones(cap), tree_cap)
    assert np.array_equal(st["sum_tree"], want_s)
    assert np.array_equal(st["min_tree"], want_m)


# ---------------------------------------------------------------------------
# the philox streams, value by value
# ---------------------------------------------------------------------------

SEED = 77


def test_reset_stream_exact():
    M, N, HOR = 64, 1, 2
    eng, _ = make_engine(capacity=M * HOR, seed=5)
    eng.rollout_alloc(M, N, horizon=HOR, eps=0.0, seed=SEED)
    eng.rollout_run(1, reset=True, use_graph=False)
    s = _state(eng)["s"][:M]
    th, td = map(np.array, zip(*[orc.roll_reset_state(SEED, 1, i)
                                 for i in range(M)]))
    assert np.abs(th).max() <= np.pi and np.abs(td).max() <= 1.0
    assert len(np.unique(np.stack([th, td], 1), axis=0)) == M
    want = np.stack([np.cos(th.astype(np.float64)),
                     np.sin(th.astype(np.float64)),
                     td.astype(np.float64)], 1)
    print(f"reset state: max abs err {np.abs(s - want).max():.3g}")
    # float32 cosf/sinf against float64 on |x| <= pi
    np.testing.assert_allclose(s, want, rtol=0, atol=1e-6)
    assert len(np.unique(s, axis=0)) == M


def _policy(net, s):
    with torch.no_grad():
        return net(torch.from_numpy(np.ascontiguousarray(s))).numpy().ravel()


def test_gaussian_stream_exact():
    M, N, HOR, EPS = 64, 1, 3, 0.3
    eng, net = make_engine(capacity=M * HOR, seed=5)
    th0, td0 = _start(M, 3)

    def run(eps):
        eng.rollout_alloc(M, N, horizon=HOR, eps=eps, seed=SEED)
        eng.rollout_set_state(th0, td0)
        eng.rollout_run(1, reset=False, use_graph=False)
        st = _state(eng)
        assert st["pos"] == 0               # capacity is one episode
        return st

    a0 = run(0.0)["a"]
    st = run(EPS)
    a1 = st["a"]
    noise = np.array([[EPS * orc.n01(*orc.roll_noise_words(SEED, 1, t, i)[:2])
                       for i in range(M)] for t in range(HOR)])
    # tick 0: both runs saw the same policy output, so the difference IS
    # the noise.  float32 argument error 2 pi 6e-8 = 4e-7, times
    # |sqrt(-2 ln u)| <= 6.7, times 0.3: 8e-7, so 1e-5 has 10x margin
    inner = np.abs(a1[:M]) < 1.0
    assert inner.sum() >= 48
    d0 = (a1[:M] - a0[:M])[inner]
    print(f"tick 0: {inner.sum()} unclipped, max abs err "
          f"{np.abs(d0 - noise[0][inner]).max():.3g}")
    np.testing.assert_allclose(d0, noise[0][inner], rtol=0, atol=1e-5)
    # clipped actions sit on the bound the noise pushed them over
    assert np.array_equal(a1[:M][~inner], np.sign(
        (a0[:M] + noise[0])[~inner]).astype(np.float32))
    # ticks 1, 2: the states have diverged; take the policy output from the
    # emitted state through the torch actor (forward parity 2e-5)
    for t in (1, 2):
        rows = slice(t * M, (t + 1) * M)
        pol = np.clip(_policy(net, st["s"][rows]), -1.0, 1.0)
        inner = np.abs(a1[rows]) < 1.0
        assert inner.sum() >= 48
        dt = (a1[rows] - pol)[inner]
        print(f"tick {t}: {inner.sum()} unclipped, max abs err "
              f"{np.abs(dt - noise[t][inner]).max():.3g}")
        np.testing.assert_allclose(dt, noise[t][inner], rtol=0, atol=5e-5)


@pytest.mark.parametrize("mu", [0.0, 0.25])
def test_ou_recurrence_exact(mu):
    M, N, HOR = 64, 1, 6
    THETA, SIGMA, DT = 0.15, 0.2, 1e-2
    eng, net = make_engine(capacity=M * HOR, seed=7)
    eng.rollout_alloc(M, N, horizon=HOR, noise="ou", eps=1.0,
                      ou_theta=THETA, ou_sigma=SIGMA, ou_mu=mu, seed=SEED)
    th0, td0 = _start(M, 3)
    eng.rollout_set_state(th0, td0)
    eng.rollout_run(1, reset=False, use_graph=False)
    st = _state(eng)
    # the process starts where the device reset starts it: at mu
    x = np.full(M, mu, np.float64)
    checked = 0
    for t in range(HOR):
        z = np.array([orc.n01(*orc.roll_noise_words(SEED, 1, t, i)[:2])
                      for i in range(M)])
        x = x + THETA * (mu - x) * DT + SIGMA * np.sqrt(DT) * z
        rows = slice(t * M, (t + 1) * M)
        a = st["a"][rows]
        inner = np.abs(a) < 1.0
        got = (a - _policy(net, st["s"][rows]))[inner]
        print(f"mu={mu} tick {t}: {inner.sum()} unclipped, max abs err "
              f"{np.abs(got - x[inner]).max():.3g}")
        # a per-tick increment is about 0.02: a stuck or re-seeded state
        # is hundreds of tolerances off
        np.testing.assert_allclose(got, x[inner], rtol=0, atol=5e-5)
        checked += int(inner.sum())
    assert checked >= HOR * M // 2
    assert np.abs(x - mu).max() > 0.02
