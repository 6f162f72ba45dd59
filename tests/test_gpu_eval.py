"""Device greedy evaluation (ops/hip/engine_eval.hip) against its host twin
vector_evaluate (d4pg_amd/envs/vector.py) driven by the philox oracles, its
freedom from side effects on everything training reads, determinism under
graph replay, the result reduction and the refusals.

Tolerances are the per-step reward bounds of the rollout parity tests summed
over the horizon: Pendulum 10 * 5e-3 + 2e-3 |ret|
(test_gpu_rollout.py::test_rollout_dynamics_and_fold_parity), synthetic
horizon * 2e-4 (ATOL of test_gpu_synth_rollout.py).  Goal returns, lengths
and success flags are exact under the margin condition of
test_gpu_goal_rollout.py, asserted on the oracle alone.

Measured on an MI355X, max |ret_dev - ret_twin|: see PARITY.md.
"""

import functools

import numpy as np
import pytest
import torch

import _engine_kit as kit
import _oracles as orc
import _synth_oracles as so
from d4pg_amd.envs.vector import (PhiloxProcNoise, VectorGoalReach,
                                  VectorPendulum, VectorSynthetic,
                                  vector_evaluate)

pytestmark = pytest.mark.gpu

H, K = 64, 51
SEED = 9                                # rollout seed
EVAL_XOR = 0x5EEDE7A1                   # default evaluation seed rule
SEED_EVAL = SEED ^ EVAL_XOR
ENV_SEED = 5                            # names the synthetic env's W, U
MARGIN = 1e-3
DIST = {"type": "categorical", "v_min": -50.0, "v_max": 1.0, "n_atoms": K}


@functools.lru_cache(maxsize=None)
def _net(o, a, seed=4, gain=60.0):
    # the gain spreads the actions over (-1, 1)
    return kit.producer_nets(o, a, DIST, hidden=H, actor_seed=seed,
                             critic_seed=1, head_gain=gain)[0]


def make_engine(o, a, capacity=1024, prioritized=True, net=None):
    return kit.producer_engine(
        o, a, hidden=H, n_atoms=K, capacity=capacity, batch=64, seed=0,
        v_min=-50.0, v_max=1.0, gamma_n=0.99 ** 3, lr=1e-3,
        prioritized=prioritized, actor_seed=4, critic_seed=1, head_gain=60.0,
        actor=net)[0]


def _synth_vec(o, a, m, hor, proc_noise=None, sigma=0.01):
    return VectorSynthetic(m, o, a, horizon=hor, act_high=0.7, seed=ENV_SEED,
                           proc_sigma=sigma, proc_noise=proc_noise)


def alloc_rollout(eng, kind, m=4, n=3, hor=10, noise="gaussian", o=None,
                  a=None):
    if kind == "pendulum":
        eng.rollout_alloc(m, n, horizon=hor, noise=noise, seed=SEED)
    elif kind == "goal":
        eng.goal_rollout_alloc(m, n, horizon=hor, speed=0.1, tol=0.3,
                               noise=noise, seed=SEED)
    else:
        vec = _synth_vec(o, a, 1, hor)
        eng.synth_rollout_alloc(m, n, vec.W, vec.U, horizon=hor,
                                act_high=0.7, proc_sigma=0.01, noise=noise,
                                seed=SEED)


# ---------------------------------------------------------------------------
# 1-3: parity against the twin
# ---------------------------------------------------------------------------

# 520: past 512 rows the policy chain takes the MFMA forward kernel
@pytest.mark.parametrize("E", [8, 260, 520])
def test_pendulum_parity(E):
    hor = 10
    eng = make_engine(3, 1)
    alloc_rollout(eng, "pendulum", hor=hor)
    eng.eval_alloc(E, horizon=hor)
    assert eng.eval_info()["seed"] == SEED_EVAL
    got = eng.evaluate(1)
    ret, length, succ = eng.eval_returns()
    # the reset kernel ran: episode 1 of the evaluation's own stream
    assert eng.eval_results()["episode"] == 1
    start = np.array([orc.roll_reset_state(SEED_EVAL, 1, i)
                      for i in range(E)], np.float64)
    vec = VectorPendulum(E, horizon=hor)
    vec.th, vec.thdot, vec.t = start[:, 0].copy(), start[:, 1].copy(), 0
    want, (wret, wlen, _) = vector_evaluate(_net(3, 1), vec, reset=False)
    err = np.abs(ret - wret)
    print(f"pendulum E={E}: max |ret_dev - ret_twin| {err.max():.3g} "
          f"(|ret| up to {np.abs(wret).max():.3g})")
    assert (err <= hor * 5e-3 + 2e-3 * np.abs(wret)).all()
    assert np.array_equal(length, wlen) and (succ == 0).all()
    assert got["env_steps"] == E * hor and got["success_rate"] == 0.0
    assert abs(got["mean_return"] - want["mean_return"]) <= \
        hor * 5e-3 + 2e-3 * abs(want["mean_return"])
    assert np.ptp(wret) > 1.0           # the envs differ


# (5, 3) at E = 520: the policy chain and the mixing GEMM on the MFMA path
@pytest.mark.parametrize("o,a,E", [(17, 6, 6), (5, 3, 6), (17, 6, 70),
                                   (5, 3, 70), (5, 3, 520)])
def test_synthetic_parity(o, a, E):
    hor = 6
    eng = make_engine(o, a)
    alloc_rollout(eng, "synth", hor=hor, o=o, a=a)
    eng.eval_alloc(E, horizon=hor)
    got = eng.evaluate(1)
    ret, length, succ = eng.eval_returns()
    vec = _synth_vec(o, a, E, hor, PhiloxProcNoise(SEED_EVAL, 1))
    vec.set_state(so.reset_state(SEED_EVAL, 1, E, o))
    want, (wret, wlen, _) = vector_evaluate(_net(o, a), vec, reset=False)
    err = np.abs(ret - wret)
    print(f"synthetic ({o}, {a}) E={E}: max |ret_dev - ret_twin| "
          f"{err.max():.3g}")
    assert err.max() <= hor * 2e-4
    assert np.array_equal(length, wlen) and (succ == 0).all()
    assert got["env_steps"] == E * hor
    # the process noise is in the returns: the noiseless twin is far off
    quiet = _synth_vec(o, a, E, hor, sigma=0.0)
    quiet.set_state(so.reset_state(SEED_EVAL, 1, E, o))
    qret = vector_evaluate(_net(o, a), quiet, reset=False)[1][0]
    assert np.abs(qret - wret).max() > 10 * err.max()


def _goal_oracle(net, pos0, goal0, hor, tol):
    vec = VectorGoalReach(len(pos0), dim=pos0.shape[1], speed=0.1, tol=tol,
                          horizon=hor)
    vec.set_state(pos0, goal0)
    out = vector_evaluate(net, vec, reset=False)
    margins = [abs(np.linalg.norm(vec.ep_pos[t + 1, i].astype(np.float64)
                                  - goal0[i]) - tol)
               for i in range(len(pos0)) for t in range(int(vec.len[i]))]
    return out, min(margins)


def test_goal_parity_exact():
    d, E, hor, tol = 2, 16, 12, 0.3
    net = _net(2 * d, d, gain=200.0)
    rng = np.random.default_rng(2)
    for _ in range(300):
        pos0 = rng.uniform(-0.6, 0.6, (E, d)).astype(np.float32)
        goal0 = np.clip(pos0 + rng.uniform(-0.7, 0.7, (E, d)), -1.0,
                        1.0).astype(np.float32)
        (want, (wret, wlen, wsucc)), margin = _goal_oracle(net, pos0, goal0,
                                                           hor, tol)
        if margin > MARGIN and wsucc.any() and (wlen == hor).any() \
                and not wsucc.all():
            break
    # on the oracle alone, before the device is looked at
    assert margin > MARGIN, "misconfigured test: a distance too near tol"
    assert wsucc.any() and ((wlen == hor) & (wsucc == 0)).any()
    eng = make_engine(2 * d, d, net=net)
    alloc_rollout(eng, "goal", hor=hor)
    eng.eval_alloc(E, horizon=hor)
    eng.eval_set_state(pos0, goal0)
    got = eng.evaluate(1)
    ret, length, succ = eng.eval_returns()
    assert np.array_equal(length, wlen)
    assert np.array_equal(succ, wsucc)
    assert np.array_equal(ret, wret)
    assert got["success_rate"] == wsucc.sum() / E
    assert got["env_steps"] == int(wlen.sum())
    assert got["mean_return"] == want["mean_return"]


# ---------------------------------------------------------------------------
# 4: no side effects
# ---------------------------------------------------------------------------

def _bytes(x):
    if isinstance(x, torch.Tensor):
        x = x.numpy()
    return np.ascontiguousarray(x).tobytes()


def _training_state(eng):
    st = eng.ext.replay_state(eng.h)
    out = {"replay." + k: _bytes(np.asarray(v)) for k, v in dict(st).items()}
    out.update({"cnt." + k: _bytes(np.float64(v))
                for k, v in dict(eng.counters()).items()})
    out.update({"slab." + k: _bytes(eng.store_slab(k)) for k in eng.SLABS})
    out["words"] = _bytes(eng.rollout_words())
    return out


@pytest.mark.parametrize("kind,prioritized", [
    ("pendulum", True), ("pendulum", False), ("goal", True), ("synth", True)])
def test_no_side_effects(kind, prioritized):
    o, a = {"pendulum": (3, 1), "goal": (4, 2), "synth": (5, 3)}[kind]

    def build():
        eng = make_engine(o, a, prioritized=prioritized)
        alloc_rollout(eng, kind, m=8, n=3, hor=10, noise="ou", o=o, a=a)
        eng.synth_fill(256, seed=7)
        run = {"pendulum": eng.rollout_run, "goal": eng.goal_rollout_run,
               "synth": eng.synth_rollout_run}[kind]
        run(1)
        eng.step(2)
        return eng, run

    def across(state):
        # the reported loss scalars are unordered float sums over the batch:
        # equal on one engine before and after, not across two engines
        return {k: v for k, v in state.items() if not k.startswith("cnt.loss")}

    eng, run = build()
    twin, twin_run = build()
    before = _training_state(eng)
    assert across(before) == across(_training_state(twin))
    eng.eval_alloc(70, horizon=7)
    got = eng.evaluate(2)
    assert got["episodes"] == 2 and np.isfinite(got["mean_return"])
    after = _training_state(eng)
    for k in before:
        assert before[k] == after[k], k
    # obs, env state, OU state and the rings were untouched: the rollout
    # goes on exactly as on the engine that did not evaluate
    run(1, reset=False)
    twin_run(1, reset=False)
    a_state = across(_training_state(eng))
    b_state = across(_training_state(twin))
    for k in a_state:
        assert a_state[k] == b_state[k], k
    assert a_state["replay.s"] != before["replay.s"]


# ---------------------------------------------------------------------------
# 5: determinism
# ---------------------------------------------------------------------------

def _snapshot(eng, **kw):
    eng.evaluate(1, **kw)
    return ([_bytes(x) for x in eng.eval_returns()],
            sorted(eng.eval_results().items()))


def test_determinism_graph_and_fixed_starts():
    eng = make_engine(3, 1)
    alloc_rollout(eng, "pendulum")
    eng.eval_alloc(70, horizon=5, fixed_starts=True)
    g1 = _snapshot(eng, use_graph=True)
    u1 = _snapshot(eng, use_graph=False)
    g2 = _snapshot(eng, use_graph=True)
    assert g1 == u1 == g2
    ret1 = eng.eval_returns()[0].copy()
    other = _net(3, 1, seed=11)
    from d4pg_amd.ops import pack_net
    eng.load_slab("actor", pack_net(other))
    eng.evaluate(1)
    ret2 = eng.eval_returns()[0]
    assert eng.eval_results()["episode"] == 1
    assert np.abs(ret2 - ret1).max() > 1e-3     # same starts, other policy
    # moving starts: the epoch advances once per episode
    eng.eval_alloc(70, horizon=5, fixed_starts=False)
    a = _snapshot(eng)
    b = _snapshot(eng)
    assert a[0][0] != b[0][0]
    assert dict(a[1])["episode"] == 1 and dict(b[1])["episode"] == 2
    r = eng.evaluate(3)
    assert eng.eval_results()["episode"] == 5 and r["env_steps"] == 3 * 70 * 5


@pytest.mark.parametrize("kind,o,a,E", [("goal", 4, 2, 70),
                                        ("synth", 5, 3, 70),
                                        ("synth", 5, 3, 520)])
def test_graph_equals_uncaptured_goal_and_synth(kind, o, a, E):
    """The goal tick's alive mask and the synthetic tick (one wave per env,
    process noise on; MFMA forwards at E = 520): a graph replay against the
    uncaptured launches, from the same fixed starts."""
    net = _net(o, a, gain=200.0) if kind == "goal" else None
    eng = make_engine(o, a, net=net)
    alloc_rollout(eng, kind, hor=8, o=o, a=a)
    eng.eval_alloc(E, horizon=8, fixed_starts=True)
    g1 = _snapshot(eng, use_graph=True)
    u1 = _snapshot(eng, use_graph=False)
    g2 = _snapshot(eng, use_graph=True)
    assert g1 == u1 == g2
    ret, length, succ = eng.eval_returns()
    assert np.ptp(ret) > 0
    if kind == "goal":                  # some envs stopped early, some not
        assert 0 < succ.sum() < E and (length[succ == 1] <= 8).all()
        assert (length[succ == 0] == 8).all()


# ---------------------------------------------------------------------------
# 6: reduce edges
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pendulum_engine():
    eng = make_engine(3, 1)
    alloc_rollout(eng, "pendulum")
    return eng


@pytest.mark.parametrize("E", [1, 63, 64, 65, 257, 1000])
def test_reduce_edges(pendulum_engine, E):
    eng = pendulum_engine
    eng.eval_alloc(E, horizon=2)
    got = eng.evaluate(1)
    ret, length, succ = eng.eval_returns()
    assert ret.shape == (E,) and (ret < 0).all()        # one sign
    assert got["min_return"] == ret.min()
    assert got["max_return"] == ret.max()
    assert got["success_rate"] == 0.0 and succ.sum() == 0
    assert got["env_steps"] == 2 * E == int(length.sum())
    mean = np.sum(ret, dtype=np.float64) / E
    assert abs(got["mean_return"] - mean) <= 1e-12 * abs(mean)


# ---------------------------------------------------------------------------
# 7: refusals
# ---------------------------------------------------------------------------

def test_refusals():
    eng = make_engine(3, 1)
    with pytest.raises(RuntimeError, match="no rollout allocated"):
        eng.eval_alloc(8)
    with pytest.raises(RuntimeError, match="eval_alloc first"):
        eng.evaluate()
    alloc_rollout(eng, "pendulum")
    for bad in (0, 65537):
        with pytest.raises(RuntimeError, match="n_envs"):
            eng.eval_alloc(bad)
    with pytest.raises(RuntimeError, match="horizon"):
        eng.eval_alloc(8, horizon=(1 << 20) - 2)
    with pytest.raises(RuntimeError, match="eval_alloc first"):
        eng.evaluate()
    eng.eval_alloc(8, horizon=3)
    # no episode, no result: refused by the engine, not only by the wrapper
    for bad in (0, -1):
        with pytest.raises(RuntimeError, match="episodes < 1"):
            eng.ext.eval_run(eng.h, bad, True)
    assert eng.evaluate()["env_steps"] == 24
    # horizon None: the rollout's
    eng.eval_alloc(8)
    assert eng.eval_info()["horizon"] == 10
    # a new rollout drops the evaluation, which modelled the old one
    alloc_rollout(eng, "pendulum")
    with pytest.raises(RuntimeError, match="eval_alloc first"):
        eng.evaluate()
    eng.eval_alloc(8, horizon=3, seed=123)
    assert eng.eval_info()["seed"] == 123
    assert eng.evaluate()["env_steps"] == 24
