"""Overlapped collection (ops/hip/engine_stage.hip, Engine::collect_*): a
window's episodes run on the rollout stream into a staging store while the
learner stream trains; collect_commit moves the rows into the live ring.

Engines: A is the engine under test; B a same-seed engine that never
collects; C a producer-only engine with an empty replay and the same rollout
seed, loaded with the actor A snapshotted.  Everything is compared bitwise
(the staged episodes launch the sync path's kernels on other pointers, and
the commit is a copy), except the new tree leaves against numpy's pow: 2 ulp.

The two loss scalars of the counters are unordered float sums over the batch
(equal on one engine before and after, not across two engines — as in
test_gpu_eval.py::test_no_side_effects) and are left out of cross-engine
comparisons.
"""

import functools

import numpy as np
import pytest
import torch

import _engine_kit as kit
import _oracles as orc
from d4pg_amd.envs.vector import VectorGoalReach, VectorSynthetic

pytestmark = pytest.mark.gpu

H, K, CAP, FILL = 64, 11, 4096, 1500
SEED = 9                                # rollout seed (see test_goal_seed_*)
ENV_SEED = 5                            # names the synthetic env's W, U
MP0 = 0.37                              # max_priority before training
ALPHA = np.float64(np.float32(0.6))     # the engine holds per_alpha as float
DIST = {"type": "categorical", "v_min": -50.0, "v_max": 1.0, "n_atoms": K}
ARR = ("s", "a", "r", "s2", "d")

# kind -> (obs, act, M, horizon, n)
KINDS = {"pendulum": (3, 1, 64, 8, 3), "goal": (4, 2, 64, 6, 2),
         "synth": (5, 2, 64, 6, 2),
         # 520 envs: the policy chain on the MFMA forward, edge tile
         "pendulum520": (3, 1, 520, 4, 3)}
GOAL_SPEED, GOAL_TOL = 0.1, 0.3


@functools.lru_cache(maxsize=None)
def _nets(o, a):
    # head times 60: spread the actions over (-1, 1)
    return kit.producer_nets(o, a, DIST, hidden=H, actor_seed=4,
                             critic_seed=1, head_gain=60.0)


def make_engine(o, a, batch=64, prioritized=True):
    return kit.producer_engine(
        o, a, hidden=H, n_atoms=K, capacity=CAP, batch=batch, seed=0,
        v_min=-50.0, v_max=1.0, gamma_n=0.99 ** 3, lr=1e-3,
        prioritized=prioritized, actor_seed=4, critic_seed=1,
        head_gain=60.0)[0]


def alloc(eng, kind):
    o, a, m, hor, n = KINDS[kind]
    if kind.startswith("pendulum"):
        eng.rollout_alloc(m, n, horizon=hor, seed=SEED)
        return eng.rollout_run
    if kind == "goal":
        eng.goal_rollout_alloc(m, n, horizon=hor, speed=GOAL_SPEED,
                               tol=GOAL_TOL, her_ratio=0.8, seed=SEED)
        return eng.goal_rollout_run
    vec = VectorSynthetic(1, o, a, horizon=hor, act_high=0.7, seed=ENV_SEED,
                          proc_sigma=0.01)
    eng.synth_rollout_alloc(m, n, vec.W, vec.U, horizon=hor, act_high=0.7,
                            proc_sigma=0.01, seed=SEED)
    return eng.synth_rollout_run


def fill(eng, o, a, ingest):
    """synth_fill, a max_priority that is not 1, then `ingest` host rows."""
    eng.synth_fill(FILL, seed=7)
    if eng.prioritized:
        eng.set_schedule(0, MP0)
    if ingest:
        rng = np.random.default_rng(3)
        t = lambda *s: torch.from_numpy(              # noqa: E731
            rng.uniform(-1, 1, s).astype(np.float32))
        eng.ingest(t(ingest, o), t(ingest, a), t(ingest), t(ingest, o),
                   torch.zeros(ingest))


def arrays(eng, base=0, count=CAP):
    return dict(zip(ARR, (x.numpy() for x in
                          eng.ext.replay_slice(eng.h, base, count))))


def cnt_words(eng):
    return {k: v for k, v in dict(eng.counters()).items()
            if not k.startswith("loss")}


def learner_state(eng):
    """Everything the train step reads or writes, through accessors that
    stay legal inside a window."""
    out = {"slab." + k: eng.store_slab(k).numpy().tobytes()
           for k in eng.SLABS}
    out["sum_tree"] = eng.read("sum_tree").numpy().tobytes()
    out["min_tree"] = eng.read("min_tree").numpy().tobytes()
    out.update({"replay." + k: v.tobytes() for k, v in arrays(eng).items()})
    out.update({"cnt." + k: repr(v) for k, v in cnt_words(eng).items()})
    return out


def train(eng, batch, n=4):
    if batch == 300:                    # row-block: through its hipGraph
        eng.train_steps(n, steps_per_graph=n)
    else:
        eng.step(n)


# ---------------------------------------------------------------------------
# 1: the learner does not see an open window
# ---------------------------------------------------------------------------

# 64: persistent kernel; 300: row-block via train_steps' graph; 640: wide
@pytest.mark.parametrize("batch", [64, 300, 640])
def test_learner_isolation(batch):
    a_eng, b_eng = make_engine(3, 1, batch), make_engine(3, 1, batch)
    for e in (a_eng, b_eng):
        fill(e, 3, 1, 0)
    alloc(a_eng, "pendulum")
    a_eng.collect_alloc(2)
    assert a_eng.info()["collect_max_episodes"] == 2
    assert b_eng.info()["collect_max_episodes"] == 0
    a_eng.collect_begin(2)
    train(a_eng, batch)
    train(b_eng, batch)
    assert a_eng.collect_pending() and not b_eng.collect_pending()
    got, want = learner_state(a_eng), learner_state(b_eng)
    assert got.keys() == want.keys()
    for k in want:
        assert got[k] == want[k], k
    assert int(a_eng.counters()["adam_t_actor"]) == 4
    env_steps, rows = a_eng.collect_commit()
    assert (env_steps, rows) == (2 * 64 * 8, 2 * 64 * 6)
    assert not a_eng.collect_pending()
    assert int(a_eng.counters()["size"]) == FILL + rows


# ---------------------------------------------------------------------------
# 2-5: snapshot semantics, rows, trees — one window per producer
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def window(kind, prioritized=True):
    """One window on A around four train steps, against B and C.  The ring
    position is moved to CAP - 200 first, so the block crosses the ring's
    end."""
    o, a, m, hor, n = KINDS[kind]
    ingest = CAP - 200 - FILL
    a_eng = make_engine(o, a, prioritized=prioritized)
    b_eng = make_engine(o, a, prioritized=prioritized)
    for e in (a_eng, b_eng):
        fill(e, o, a, ingest)
    alloc(a_eng, kind)
    a_eng.collect_alloc(2)
    r = dict(kind=kind, m=m, hor=hor, n=n)
    snap = a_eng.store_slab("actor")
    a_eng.collect_begin(2)
    a_eng.step(4)
    b_eng.step(4)
    r["actor_moved"] = not torch.equal(a_eng.store_slab("actor"), snap)
    r["snap_kept"] = torch.equal(a_eng.read("p_actor_roll"), snap)
    r["cnt0"] = dict(a_eng.counters())          # just before the commit
    r["out"] = a_eng.collect_commit()
    r["cnt1"] = dict(a_eng.counters())
    r["last"] = tuple(int(x) for x in a_eng.ext.rollout_last(a_eng.h))
    r["words_a"] = a_eng.rollout_words().copy()
    r["A"], r["B"] = arrays(a_eng), arrays(b_eng)
    r["b_cnt"] = dict(b_eng.counters())
    r["tree_cap"] = int(a_eng.info()["tree_cap"])
    for t in ("sum_tree", "min_tree"):
        r["A." + t] = a_eng.read(t).numpy()
        r["B." + t] = b_eng.read(t).numpy()
    c_eng = make_engine(o, a, prioritized=prioritized)
    run = alloc(c_eng, kind)
    c_eng.load_slab("actor", snap)
    r["c_out"] = tuple(run(2))
    r["c_size"] = int(c_eng.counters()["size"])
    r["C"] = arrays(c_eng, 0, r["c_size"])
    r["words_c"] = c_eng.rollout_words().copy()
    return r


def check_rows(r):
    # otherwise the comparison with C shows nothing about the snapshot
    assert r["actor_moved"] and r["snap_kept"]
    env_steps, rows = r["out"]
    pos0 = int(r["cnt0"]["pos"])
    assert pos0 == CAP - 200 and rows > 200      # the block wraps
    assert rows == r["c_size"] and (env_steps, rows) == r["c_out"][:2]
    slots = (pos0 + np.arange(rows)) % CAP
    for k in ARR:
        assert np.array_equal(r["A"][k][slots], r["C"][k]), k
    rest = np.setdiff1d(np.arange(CAP), slots)
    for k in ARR:
        assert np.array_equal(r["A"][k][rest], r["B"][k][rest]), k
    assert int(r["cnt1"]["pos"]) == (pos0 + rows) % CAP
    assert int(r["cnt1"]["size"]) == min(int(r["cnt0"]["size"]) + rows, CAP)
    # rollout_last_rows(): the committed block from its live base
    assert r["last"] == (pos0, rows)
    # episodes continue the producer's philox epoch
    assert r["words_a"][0] == r["words_c"][0] == 2
    return slots, rest


@pytest.mark.parametrize("kind", ["pendulum", "pendulum520"])
def test_snapshot_and_rows(kind):
    r = window(kind)
    check_rows(r)
    assert r["out"] == (2 * r["m"] * r["hor"],
                        2 * r["m"] * (r["hor"] - r["n"] + 1))


def test_trees():
    r = window("pendulum")
    slots, rest = check_rows(r)
    tc = r["tree_cap"]
    mp = np.float32(r["cnt0"]["max_priority"])
    assert mp != np.float32(1.0) and mp >= np.float32(MP0)
    want = np.float64(mp) ** ALPHA
    st, mt = r["A.sum_tree"], r["A.min_tree"]
    new = st[tc + slots]
    assert (new == new[0]).all() and (mt[tc + slots] == new[0]).all()
    assert abs(new[0] - want) <= 2 * np.spacing(want)
    for t in ("sum_tree", "min_tree"):
        assert np.array_equal(r["A." + t][tc + rest], r["B." + t][tc + rest])
        assert np.array_equal(r["A." + t][tc + CAP:], r["B." + t][tc + CAP:])
    node = np.arange(1, tc)
    assert np.array_equal(st[node], st[2 * node] + st[2 * node + 1])
    assert np.array_equal(mt[node], np.minimum(mt[2 * node],
                                               mt[2 * node + 1]))
    # the ring as a plain numpy ring: B's state, then the new rows
    ring = orc.RingOracle(CAP, tc)
    ring.rows = {k: r["B"][k].copy() for k in ARR}
    ring.rows["r"], ring.rows["d"] = (ring.rows["r"].ravel(),
                                      ring.rows["d"].ravel())
    ring.leaves = r["B.sum_tree"][tc:tc + CAP].copy()
    ring.size, ring.pos = int(r["b_cnt"]["size"]), int(r["b_cnt"]["pos"])
    ring.add(*(r["C"][k] for k in ARR), leaf=new[0])
    for k in ARR:
        assert np.array_equal(ring.rows[k].ravel(), r["A"][k].ravel()), k
    assert ring.size == int(r["cnt1"]["size"])
    assert ring.pos == int(r["cnt1"]["pos"])
    assert np.array_equal(ring.leaves, st[tc:tc + CAP])
    assert np.array_equal(ring.leaves, mt[tc:tc + CAP])


def _goal_starts(seed, ep, m, d):
    f = np.float32
    p, g = np.zeros((m, d), f), np.zeros((m, d), f)
    for i in range(m):
        for k in range(d):
            v = orc.philox4x32_10(seed ^ 0xD011E, (ep << 20) | 1,
                                  (k << 32) | i)
            p[i, k] = f(f(2.0) * orc.u01(v[0]) - f(1.0))
            g[i, k] = f(f(2.0) * orc.u01(v[1]) - f(1.0))
    return p, g


def test_goal_seed_has_early_and_late_envs():
    """CPU only: rollout seed 9 gives, in both episodes of the window, envs
    that succeed at their first step whatever the policy does (start within
    tol - speed * sqrt(D) of the goal: 1 and 2 envs) and envs that cannot
    succeed within the horizon (start further than tol + horizon * speed *
    sqrt(D): 27 and 25 envs).  Checked with VectorGoalReach under the worst
    policy for the first kind and the best for the second."""
    o, a, m, hor, n = KINDS["goal"]
    for ep, n_early, n_never in ((1, 1, 27), (2, 2, 25)):
        p, g = _goal_starts(SEED, ep, m, a)
        dist = np.linalg.norm(p.astype(np.float64) - g, axis=1)
        reach = GOAL_SPEED * np.sqrt(a)
        early = dist <= GOAL_TOL - reach - 1e-3
        never = dist > GOAL_TOL + hor * reach + 1e-3
        assert (early.sum(), never.sum()) == (n_early, n_never)
        vec = VectorGoalReach(m, dim=a, speed=GOAL_SPEED, tol=GOAL_TOL,
                              horizon=hor)
        vec.set_state(p, g)
        for _ in range(hor):
            toward = np.clip((vec.goal - vec.pos) / GOAL_SPEED, -1.0, 1.0)
            away = np.sign(vec.pos - vec.goal)
            vec.step(np.where(early[:, None], away, toward))
        assert (vec.succ[early] & (vec.len[early] == 1)).all()
        assert not vec.succ[never].any() and (vec.len[never] == hor).all()


@pytest.mark.parametrize("kind", ["goal", "synth"])
def test_goal_and_synth_producers(kind):
    r = window(kind)
    check_rows(r)
    if kind == "goal":
        m, hor = r["m"], r["hor"]
        # device totals of the window, equal to C's run totals
        assert tuple(r["words_a"][5:8]) == tuple(r["words_c"][5:8])
        rows, succ, steps = (int(x) for x in r["words_a"][5:8])
        assert (steps, rows) == r["out"] and r["c_out"][2] == succ
        # some envs stopped early, some ran to the limit (seed 9, above)
        assert 3 <= succ <= 2 * m - 52 and steps < 2 * m * hor
    else:
        assert r["out"] == (2 * r["m"] * r["hor"],
                            2 * r["m"] * (r["hor"] - r["n"] + 1))


def test_uniform_replay():
    r = window("pendulum", prioritized=False)
    check_rows(r)
    assert r["tree_cap"] == 0
    assert r["A.sum_tree"].size == 0 and r["A.min_tree"].size == 0
    assert float(r["cnt1"]["max_priority"]) == float(r["b_cnt"]
                                                     ["max_priority"])


# ---------------------------------------------------------------------------
# 6: two windows, mixing with the sync path, graph against uncaptured
# ---------------------------------------------------------------------------

def _replay_bytes(eng):
    st = dict(eng.ext.replay_state(eng.h))
    return {k: np.ascontiguousarray(np.asarray(v)).tobytes()
            for k, v in st.items()}


@pytest.mark.parametrize("kind", ["pendulum", "goal"])
def test_two_windows_and_sync_mix(kind):
    o, a, m, hor, n = KINDS[kind]
    a_eng, c_eng = make_engine(o, a), make_engine(o, a)
    run_a, run_c = alloc(a_eng, kind), alloc(c_eng, kind)
    a_eng.collect_alloc(2)
    a_eng.collect_begin(2)
    out1 = a_eng.collect_commit()
    a_eng.collect_begin(1, use_graph=False)
    out2 = a_eng.collect_commit()
    out3 = run_a(1)
    want = [run_c(2), run_c(1), run_c(1)]
    assert [tuple(out1), tuple(out2), tuple(out3)[:2]] == \
        [tuple(w)[:2] for w in want]
    got, ref = _replay_bytes(a_eng), _replay_bytes(c_eng)
    for k in ref:
        assert got[k] == ref[k], k
    assert np.array_equal(a_eng.rollout_words(), c_eng.rollout_words())
    assert a_eng.rollout_words()[0] == 4            # epochs continue


@pytest.mark.parametrize("kind", ["pendulum", "goal", "synth"])
def test_graph_equals_uncaptured(kind):
    o, a, m, hor, n = KINDS[kind]
    res = []
    for use_graph in (True, False):
        eng = make_engine(o, a)
        alloc(eng, kind)
        eng.collect_alloc(2)
        eng.collect_begin(2, use_graph=use_graph)
        out = eng.collect_commit()
        res.append((out, _replay_bytes(eng), eng.rollout_words().tobytes(),
                    eng.read("stage_s").numpy().tobytes()))
    assert res[0] == res[1]
    assert res[0][0][1] > 0


# ---------------------------------------------------------------------------
# 7: refusals
# ---------------------------------------------------------------------------

def test_refusals_outside_a_window():
    eng = make_engine(3, 1)
    with pytest.raises(RuntimeError, match="no rollout allocated"):
        eng.collect_alloc(2)
    with pytest.raises(RuntimeError, match="collect_alloc first"):
        eng.collect_begin(1)
    with pytest.raises(RuntimeError, match="no collection window is open"):
        eng.collect_commit()
    alloc(eng, "pendulum")
    with pytest.raises(RuntimeError, match="collect_alloc first"):
        eng.collect_begin(1)
    for bad in (0, -3):
        with pytest.raises(RuntimeError, match="max_episodes < 1"):
            eng.collect_alloc(bad)
    # 11 episodes x 384 rows = 4224 > 4096
    with pytest.raises(RuntimeError, match="two rows to one slot"):
        eng.collect_alloc(11)
    with pytest.raises(RuntimeError, match="unknown buffer"):
        eng.read("p_actor_roll")
    eng.collect_alloc(10)
    for bad in (0, 11, 1 << 40):
        with pytest.raises(RuntimeError, match="episodes not in"):
            eng.collect_begin(bad)
    assert not eng.collect_pending()
    with pytest.raises(RuntimeError, match="no collection window is open"):
        eng.collect_commit()
    # a new producer frees the staging store
    alloc(eng, "pendulum")
    assert eng.info()["collect_max_episodes"] == 0
    with pytest.raises(RuntimeError, match="collect_alloc first"):
        eng.collect_begin(1)


@pytest.mark.parametrize("kind", ["pendulum", "goal", "synth"])
def test_refusals_inside_a_window(kind):
    o, a, m, hor, n = KINDS[kind]
    eng, c_eng = make_engine(o, a), make_engine(o, a)
    run = alloc(eng, kind)
    run_c = alloc(c_eng, kind)
    fill(eng, o, a, 0)
    eng.collect_alloc(2)
    state = dict(eng.ext.replay_state(eng.h))
    eng.collect_begin(2)
    z = np.zeros((m, a), np.float32)
    set_state = {
        "pendulum": lambda: eng.rollout_set_state(z[:, 0], z[:, 0]),
        "goal": lambda: eng.goal_rollout_set_state(z, z),
        "synth": lambda: eng.synth_rollout_set_state(
            np.zeros((m, o), np.float32))}[kind]
    refused = [
        lambda: run(1), set_state, lambda: alloc(eng, kind),
        # (another producer's allocator, legal at any obs/act size)
        lambda: eng.synth_rollout_alloc(
            m, n, np.eye(o, dtype=np.float32), np.zeros((a, o), np.float32),
            horizon=hor, seed=SEED),
        lambda: eng.collect_begin(1), lambda: eng.collect_alloc(2),
        lambda: eng.set_seed(5), lambda: eng.ext.replay_state(eng.h),
        lambda: eng.ext.load_replay_state(
            eng.h, state["s"], state["a"], state["r"], state["s2"],
            state["d"], state["sum_tree"], state["min_tree"],
            int(state["size"]), int(state["pos"]), 1.0)]
    for call in refused:
        with pytest.raises(RuntimeError, match="collect_commit"):
            call()
        assert eng.collect_pending()
    # what stays legal
    eng.step(2)
    eng.step_part(eng.PH_CRITIC_GRADS)
    assert int(eng.counters()["adam_t_actor"]) == 2
    eng.read("bs")
    eng.rollout_words()
    # the refused calls left the window whole
    pos0 = int(eng.counters()["pos"])
    out = eng.collect_commit()
    want = run_c(2)
    assert tuple(out) == tuple(want)[:2]
    got, ref = arrays(eng, pos0, out[1]), arrays(c_eng, 0, out[1])
    for k in ARR:
        assert np.array_equal(got[k], ref[k]), k
    # and everything refused is legal again
    eng.set_seed(5)
    run(1)


# ---------------------------------------------------------------------------
# 8: evaluation inside a window
# ---------------------------------------------------------------------------

def test_evaluate_inside_a_window():
    a_eng, b_eng, c_eng = (make_engine(3, 1) for _ in range(3))
    for e in (a_eng, b_eng):
        fill(e, 3, 1, 0)
        alloc(e, "pendulum")
        e.eval_alloc(16, horizon=5)
    a_eng.collect_alloc(2)
    snap = a_eng.store_slab("actor")
    a_eng.collect_begin(2)
    a_eng.step(4)
    b_eng.step(4)
    got = a_eng.evaluate(1)
    assert a_eng.collect_pending()
    want = b_eng.evaluate(1)
    assert got == want and np.isfinite(got["mean_return"])
    assert a_eng.eval_results() == b_eng.eval_results()
    for x, y in zip(a_eng.eval_returns(), b_eng.eval_returns()):
        assert np.array_equal(x, y)
    pos0 = int(a_eng.counters()["pos"])
    out = a_eng.collect_commit()
    run_c = alloc(c_eng, "pendulum")
    c_eng.load_slab("actor", snap)
    assert tuple(out) == tuple(run_c(2))
    got, ref = arrays(a_eng, pos0, out[1]), arrays(c_eng, 0, out[1])
    for k in ARR:
        assert np.array_equal(got[k], ref[k]), k
