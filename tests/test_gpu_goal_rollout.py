"""Device goal-reaching rollout with on-device hindsight relabelling
(ops/hip/engine_goal.hip) against its host twins.

Episode parity: the device's recorded episode against VectorGoalReach driven
by the torch actor and the philox noise oracle.  Emit parity: the device's
replay rows, slot by slot, against vector_add_experience — the scalar
add_experience once per env, with PhiloxHerRng reproducing the device's HER
draws — run on the device's OWN recorded episode, so copies are compared
bitwise.

Margin condition (not a tolerance on the device): every distance the oracle
compares with `tol`, real and hindsight, except the exactly-zero fut == t
ones, must be more than 1e-3 away from it, or the test fails as
misconfigured.  That keeps float32 summation order and fma contraction from
legitimately flipping a reward, a done flag or an episode length.
"""

import numpy as np
import pytest

import _engine_kit as kit
import _oracles as orc
from _goal_oracles import (D, EPS, GAMMA, H, HOR, K, M, MARGIN, NET_SEED, SEED,
                           SPEED, TOL, _noise, assert_margin,
                           assert_rows_equal, cpu_episode, device_episode,
                           env_margins, episode_max, make_engine,
                           oracle_counts, oracle_rows, starts as _starts)

pytestmark = pytest.mark.gpu

ALPHA = np.float64(np.float32(0.6))     # the engine holds per_alpha as float


def _state(eng):
    st = eng.ext.replay_state(eng.h)
    out = {k: st[k].numpy() for k in ("s", "a", "s2", "sum_tree", "min_tree")}
    for k in ("r", "d"):
        out[k] = st[k].numpy().ravel()
    out["size"], out["pos"] = int(st["size"]), int(st["pos"])
    return out


def _run_injected(n, ratio, capacity=None, seed=SEED):
    pos0, goal0 = _starts()
    eng = make_engine(capacity or episode_max(M, n, HOR), seed=NET_SEED)
    eng.goal_rollout_alloc(M, n, horizon=HOR, gamma=GAMMA, speed=SPEED,
                           tol=TOL, her_ratio=ratio, eps=EPS, seed=seed)
    eng.goal_rollout_set_state(pos0, goal0)
    totals = eng.goal_rollout_run(1, reset=False, use_graph=False)
    return eng, totals


# ---------------------------------------------------------------------------
# episode parity
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3])
def test_episode_parity(n):
    pos0, goal0 = _starts()
    vec = cpu_episode(pos0, goal0, EPS)
    T = vec.len
    # the spread the starts were searched for
    assert 1 in T and 2 in T and HOR in T
    assert ((T >= 3) & (T < HOR)).any()
    assert (~vec.succ[T == HOR]).any() and vec.succ[T < HOR].all()
    assert_margin(vec.ep_pos, T, vec.goal, 0.8)

    eng, (env_steps, rows, successes) = _run_injected(n, 0.8)
    epi = device_episode(eng)
    assert np.array_equal(epi["len"], T)
    assert np.array_equal(epi["succ"], vec.succ.astype(np.int32))
    assert np.array_equal(epi["goal"], goal0)
    assert np.array_equal(epi["ep_pos"][0], pos0)
    worst_a = worst_p = 0.0
    for i in range(M):
        da = np.abs(epi["ep_act"][:T[i], i] - vec.ep_act[:T[i], i]).max()
        dp = np.abs(epi["ep_pos"][:T[i] + 1, i]
                    - vec.ep_pos[:T[i] + 1, i]).max()
        worst_a, worst_p = max(worst_a, da), max(worst_p, dp)
    print(f"n={n}: lengths {list(T)}; max abs err ep_act {worst_a:.3g} "
          f"ep_pos {worst_p:.3g}")
    assert worst_a <= 2e-4 and worst_p <= 2e-4
    assert env_steps == T.sum() and successes == vec.succ.sum()
    assert rows == oracle_counts(epi, n, 0.8).sum()


# ---------------------------------------------------------------------------
# emit parity and the HER ratio edges
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3])
def test_emit_parity(n):
    eng, (env_steps, rows, successes) = _run_injected(n, 0.8)
    epi = device_episode(eng)
    margin = assert_margin(epi["ep_pos"], epi["len"], epi["goal"], 0.8)
    want = oracle_rows(epi, n, 0.8)
    got = eng.rollout_last_rows()
    assert_rows_equal(got, want, n)
    print(f"n={n}: {rows} rows, margin {margin:.3g}, max |r| err "
          f"{np.abs(got[2] - want[2]).max():.3g}")
    n_real = np.maximum(0, epi["len"] - n + 1).sum()
    assert n_real < rows < n_real + epi["len"].sum()    # some HER, not all
    st = _state(eng)
    assert rows == len(want[2])
    assert (st["size"], st["pos"]) == (rows, rows % episode_max(M, n, HOR))
    assert successes == epi["succ"].sum() and env_steps == epi["len"].sum()
    info = eng.goal_rollout_info()
    assert (info["base"], info["rows"], info["episode"]) == (0, rows, 1)
    # hindsight rows are there, and the fut == t ones are terminal
    assert (want[4] == 1.0).sum() > epi["succ"].sum()
    # the occupied prefix of the ring IS the episode
    for k, w in zip(("s", "a", "r", "s2", "d"), got):
        assert np.array_equal(st[k], w), k


@pytest.mark.parametrize("n", [1, 3])
def test_her_ratio_edges(n):
    eng0, (_, rows0, _) = _run_injected(n, 0.0)
    epi0 = device_episode(eng0)
    n_real = np.maximum(0, epi0["len"] - n + 1)
    assert rows0 == n_real.sum()
    assert_margin(epi0["ep_pos"], epi0["len"], epi0["goal"], 0.0)
    assert_rows_equal(eng0.rollout_last_rows(), oracle_rows(epi0, n, 0.0), n)

    eng1, (_, rows1, _) = _run_injected(n, 1.0)
    epi1 = device_episode(eng1)
    # the ratio does not touch the episode itself
    for k in epi0:
        assert np.array_equal(epi0[k], epi1[k]), k
    assert rows1 == n_real.sum() + epi1["len"].sum()    # one per live step
    assert_margin(epi1["ep_pos"], epi1["len"], epi1["goal"], 1.0)
    got, want = eng1.rollout_last_rows(), oracle_rows(epi1, n, 1.0)
    assert_rows_equal(got, want, n)
    # env by env: the real rows of the ratio-0 run, then len[i] HER rows
    real0 = eng0.rollout_last_rows()
    lo0 = lo1 = 0
    for i in range(M):
        for x, y in zip(got, real0):
            assert np.array_equal(x[lo1:lo1 + n_real[i]],
                                  y[lo0:lo0 + n_real[i]])
        lo0 += n_real[i]
        lo1 += n_real[i] + epi1["len"][i]


# ---------------------------------------------------------------------------
# ring wrap, leaves and the per-episode tree rebuild
# ---------------------------------------------------------------------------

def test_ring_wrap_and_trees():
    # seed 6: episode 2 (philox epoch 2) clears tol by 1e-2 on the oracle
    n, cap, seed = 3, 150, 6
    per_max = episode_max(M, n, HOR)
    assert per_max == 144
    pos0, goal0 = _starts()
    eng = make_engine(cap, seed=NET_SEED)
    tree_cap = eng.info()["tree_cap"]
    assert tree_cap == 256                  # > capacity
    eng.goal_rollout_alloc(M, n, horizon=HOR, gamma=GAMMA, speed=SPEED,
                           tol=TOL, her_ratio=1.0, eps=EPS, seed=seed)
    # episode 1: goals out of reach, so every env runs to the limit
    far = np.where(pos0 > 0, -1.0, 1.0).astype(np.float32)
    eng.goal_rollout_set_state(pos0, far)
    _, rows1, succ1 = eng.goal_rollout_run(1, reset=False, use_graph=False)
    assert (rows1, succ1) == (per_max, 0)
    ep1 = _state(eng)
    assert (ep1["size"], ep1["pos"]) == (per_max, per_max)
    want_s, want_m = orc.build_trees(np.ones(per_max), tree_cap)
    assert np.array_equal(ep1["sum_tree"], want_s)
    assert np.array_equal(ep1["min_tree"], want_m)

    eng.set_schedule(0, max_priority=2.5)
    eng.goal_rollout_set_state(pos0, goal0)
    _, rows2, _ = eng.goal_rollout_run(1, reset=False, use_graph=False)
    epi = device_episode(eng)
    assert_margin(epi["ep_pos"], epi["len"], epi["goal"], 1.0, seed=seed,
                  ep=2)
    assert cap - per_max < rows2 < per_max  # crosses the end, keeps some
    st = _state(eng)
    assert (st["size"], st["pos"]) == (cap, (per_max + rows2) % cap)
    info = eng.goal_rollout_info()
    assert (info["base"], info["rows"], info["episode"]) == (per_max, rows2, 2)
    slots = (per_max + np.arange(rows2)) % cap
    want = oracle_rows(epi, n, 1.0, seed=seed, ep=2)
    assert_rows_equal(tuple(st[k][slots] for k in ("s", "a", "r", "s2", "d")),
                      want, n)
    assert_rows_equal(eng.rollout_last_rows(), want, n)
    kept = np.setdiff1d(np.arange(cap), slots)
    assert np.array_equal(kept, np.arange((per_max + rows2) % cap, per_max))
    for k in ("s", "a", "r", "s2", "d"):
        assert np.array_equal(st[k][kept], ep1[k][kept]), k

    leaves = st["sum_tree"][tree_cap:tree_cap + cap]
    assert (leaves[kept] == 1.0).all()
    new = np.float64(np.float32(2.5)) ** ALPHA
    ulps = np.abs(leaves[slots] - new) / np.spacing(new)
    print(f"2.5^alpha leaves: max {ulps.max():.0f} ulp from the host pow")
    assert (ulps <= 2).all()
    assert np.array_equal(st["min_tree"][tree_cap:tree_cap + cap], leaves)
    want_s, want_m = orc.build_trees(leaves, tree_cap)
    assert np.array_equal(st["sum_tree"], want_s)
    assert np.array_equal(st["min_tree"], want_m)


# ---------------------------------------------------------------------------
# the scan: M no multiple of the block, and more than one block's worth
# ---------------------------------------------------------------------------

# 520 and 1032 are also on the MFMA policy forward (M >= 512); 1032 gives
# the scan's 1024 threads runs of two envs with a ragged tail.
def _scan_starts(m, hor, ratio):
    """Random starts with a mix of outcomes; with thousands of distances
    some land on the threshold, so envs whose oracle episode comes within
    3x the margin of it are redrawn (envs are independent given their
    index)."""
    rng = np.random.default_rng(m)
    pos0 = np.zeros((m, D), np.float32)
    goal0 = np.zeros((m, D), np.float32)
    redo = np.arange(m)
    for _ in range(20):
        k = len(redo)
        pos0[redo] = rng.uniform(-0.5, 0.5, (k, D))
        ang = rng.uniform(0, 2 * np.pi, k)
        dist = rng.choice([0.32, 0.36, 0.42, 1.2], k)
        goal0[redo] = pos0[redo] + (dist * np.stack([np.cos(ang),
                                                     np.sin(ang)])).T
        vec = cpu_episode(pos0, goal0, EPS, hor=hor)
        redo = np.flatnonzero(env_margins(vec.ep_pos, vec.len, vec.goal,
                                          ratio) <= 3 * MARGIN)
        if len(redo) == 0:
            return pos0, goal0
    raise AssertionError("misconfigured test: no starts clear of tol")


@pytest.mark.parametrize("m", [520, 1032])
def test_scan_offsets(m):
    n, hor, ratio = 2, 4, 0.5
    pos0, goal0 = _scan_starts(m, hor, ratio)
    eng = make_engine(episode_max(m, n, hor), seed=NET_SEED)
    eng.goal_rollout_alloc(m, n, horizon=hor, gamma=GAMMA, speed=SPEED,
                           tol=TOL, her_ratio=ratio, eps=EPS, seed=SEED)
    eng.goal_rollout_set_state(pos0, goal0)
    env_steps, rows, successes = eng.goal_rollout_run(1, reset=False,
                                                      use_graph=False)
    epi = device_episode(eng)
    T = epi["len"]
    assert len(np.unique(T)) >= 3 and (T < n).any()
    assert env_steps == T.sum() and successes == epi["succ"].sum()
    counts = oracle_counts(epi, n, ratio)
    assert len(np.unique(counts)) >= 4
    offsets = np.cumsum(counts) - counts
    assert rows == counts.sum()
    s, a, r, s2, d = eng.rollout_last_rows()
    assert len(r) == rows
    # every env's block starts at its offset: all rows of the block carry
    # the env's own first action or, for HER rows, its own positions
    for i in range(m):
        if counts[i] == 0:
            continue
        blk = slice(offsets[i], offsets[i] + counts[i])
        starts = epi["ep_pos"][:T[i], i]
        assert all((starts == p).all(1).any() for p in s[blk, :D]), i
        n_real = max(0, T[i] - n + 1)
        assert np.array_equal(s[blk][:n_real, D:],
                              np.tile(epi["goal"][i], (n_real, 1))), i
    assert_margin(epi["ep_pos"], T, epi["goal"], ratio)
    assert_rows_equal((s, a, r, s2, d), oracle_rows(epi, n, ratio), n)


# ---------------------------------------------------------------------------
# graph replay == uncaptured launches
# ---------------------------------------------------------------------------

def test_graph_replay_equals_uncaptured_bitwise():
    m, n, hor = 64, 3, 8
    runs = []
    for use_graph in (True, False):
        eng = make_engine(2 * episode_max(m, n, hor), seed=NET_SEED)
        eng.goal_rollout_alloc(m, n, horizon=hor, gamma=GAMMA, speed=SPEED,
                               tol=0.5, her_ratio=0.8, eps=EPS, seed=13)
        totals = eng.goal_rollout_run(2, reset=True, use_graph=use_graph)
        runs.append((totals, _state(eng), device_episode(eng),
                     eng.goal_rollout_info()))
    (tg, sg, eg, ig), (tu, su, eu, iu) = runs
    assert tg == tu and ig == iu
    env_steps, rows, successes = tg
    assert 0 < successes < 2 * m and env_steps < 2 * m * hor
    assert (sg["size"], sg["pos"]) == (rows, rows)
    assert ig["episode"] == 2 and ig["base"] + ig["rows"] == rows
    for k in sg:
        assert np.array_equal(sg[k], su[k]), k
    for k in eg:
        assert np.array_equal(eg[k], eu[k]), k
    # the philox epoch advanced inside the graph: episode 2 is new data
    first = sg["s"][:ig["base"]]
    assert not (first[:, None, :D] == eg["ep_pos"][0][None]).all(2).any()
    leaves = sg["sum_tree"][eng.info()["tree_cap"]:][:rows]
    assert (leaves == 1.0).all()
    want_s, want_m = orc.build_trees(leaves, eng.info()["tree_cap"])
    assert np.array_equal(sg["sum_tree"], want_s)
    assert np.array_equal(sg["min_tree"], want_m)


# ---------------------------------------------------------------------------
# the philox streams: reset state, and the noise of action dim 1
# ---------------------------------------------------------------------------

def test_reset_stream_exact():
    m, n, hor = 64, 1, 2
    eng = make_engine(episode_max(m, n, hor), seed=NET_SEED)
    eng.goal_rollout_alloc(m, n, horizon=hor, speed=SPEED, tol=TOL,
                           eps=0.0, seed=SEED)
    eng.goal_rollout_run(1, reset=True, use_graph=False)
    epi = device_episode(eng)
    f = np.float32
    want_p = np.zeros((m, D), np.float64)
    want_g = np.zeros((m, D), np.float64)
    for i in range(m):
        for k in range(D):
            v = orc.philox4x32_10(SEED ^ 0xD011E, (1 << 20) | 1,
                                  (k << 32) | i)
            want_p[i, k] = f(f(2.0) * orc.u01(v[0]) - f(1.0))
            want_g[i, k] = f(f(2.0) * orc.u01(v[1]) - f(1.0))
    err = max(np.abs(epi["ep_pos"][0] - want_p).max(),
              np.abs(epi["goal"] - want_g).max())
    print(f"reset state: max abs err {err:.3g}")
    np.testing.assert_allclose(epi["ep_pos"][0], want_p, rtol=0, atol=1e-6)
    np.testing.assert_allclose(epi["goal"], want_g, rtol=0, atol=1e-6)
    assert np.abs(want_p).max() <= 1.0 and np.abs(want_g).max() <= 1.0
    assert len(np.unique(np.hstack([want_p, want_g]).ravel())) == 2 * m * D
    # every env took its first step from there, with a zeroed episode state
    assert (epi["len"] >= 1).all()


def test_gaussian_stream_exact_per_action_dim():
    m, n, hor = 64, 1, 1
    rng = np.random.default_rng(3)
    pos0 = rng.uniform(-0.5, 0.5, (m, D)).astype(np.float32)
    goal0 = -np.sign(pos0).astype(np.float32)       # far away
    eng = make_engine(episode_max(m, n, hor), seed=NET_SEED)

    def first_actions(eps):
        eng.goal_rollout_alloc(m, n, horizon=hor, speed=SPEED, tol=TOL,
                               eps=eps, seed=SEED)
        eng.goal_rollout_set_state(pos0, goal0)
        eng.goal_rollout_run(1, reset=False, use_graph=False)
        return device_episode(eng)["ep_act"][0]

    a0, a1 = first_actions(0.0), first_actions(EPS)
    noise = _noise(SEED, 1, 0, m, EPS)
    # the two dims draw different streams
    assert np.abs(noise[:, 0] - noise[:, 1]).min() > 0
    for k in range(D):
        inner = np.abs(a1[:, k]) < 1.0
        assert inner.sum() >= 48
        got = (a1[:, k] - a0[:, k])[inner]
        print(f"dim {k}: {inner.sum()} unclipped, max abs err "
              f"{np.abs(got - noise[inner, k]).max():.3g}")
        np.testing.assert_allclose(got, noise[inner, k], rtol=0, atol=5e-5)
        assert np.array_equal(a1[~inner, k], np.sign(
            (a0[:, k] + noise[:, k])[~inner]).astype(np.float32))


# ---------------------------------------------------------------------------
# refusals (host-side checks; nothing is launched)
# ---------------------------------------------------------------------------

def test_refusals():
    n = 3
    eng = make_engine(episode_max(M, n, HOR) - 1, seed=NET_SEED)
    with pytest.raises(RuntimeError, match="capacity"):
        eng.goal_rollout_alloc(M, n, horizon=HOR)
    with pytest.raises(RuntimeError, match="horizon"):
        eng.goal_rollout_alloc(1, n, horizon=n - 1)
    with pytest.raises(RuntimeError, match="goal_rollout_alloc first"):
        eng.goal_rollout_run(1)
    eng.goal_rollout_alloc(M - 1, n, horizon=HOR)      # one env fewer fits
    pend = kit.engine(kit.Shape(64, H, 3, 1, K, v_min=-50.0), capacity=4096,
                      seed=0, gamma_n=GAMMA)
    with pytest.raises(RuntimeError, match="2\\*act"):
        pend.goal_rollout_alloc(M, 1, horizon=HOR)
