"""Engine lifetime: destroying an engine, with every pool and graph live or
with a collection window open, frees only what is its own.

The destructor drains the rollout stream first, then releases graphs and
pools, then events and streams (ops/hip/engine.hip, ~Engine).  Nothing here
compares against a host oracle: engines built from the same seed, slabs and
replay fill must stay bitwise equal whatever lived and died beside them.
"""

import gc

import numpy as np
import pytest
import torch

import _engine_kit as kit
from d4pg_amd.envs.vector import VectorSynthetic

pytestmark = pytest.mark.gpu

H, K, CAP = 64, 11, 256
M, N, HOR = 5, 2, 6
GAMMA = 0.99
KINDS = ["pendulum", "goal", "synth"]


def _engine(o, batch):
    """One fixed initial state: seed, slabs and replay fill."""
    eng, _ = kit.producer_engine(
        o, 1, hidden=H, n_atoms=K, capacity=CAP, batch=batch, seed=3,
        v_min=-10.0, v_max=1.0, gamma_n=GAMMA ** N, lr=1e-4, actor_seed=4,
        critic_seed=None)
    eng.synth_fill(200, seed=7)
    return eng


def _obs(kind):
    return 2 if kind == "goal" else 3


def _alloc(eng, kind):
    if kind == "pendulum":
        eng.rollout_alloc(M, N, horizon=HOR, gamma=GAMMA, seed=21)
    elif kind == "goal":
        eng.goal_rollout_alloc(M, N, horizon=HOR, gamma=GAMMA, tol=0.3,
                               seed=21)
    else:
        vec = VectorSynthetic(M, 3, 1, horizon=HOR, seed=5)
        eng.synth_rollout_alloc(M, N, vec.W, vec.U, horizon=HOR, gamma=GAMMA,
                                seed=21)


def _run(eng, kind):
    run = {"pendulum": eng.rollout_run, "goal": eng.goal_rollout_run,
           "synth": eng.synth_rollout_run}[kind]
    return run(1, reset=True, use_graph=True)


LOSSES = ("loss_critic", "loss_actor")


def _snapshot(eng):
    st = {name: eng.store_slab(name) for name in eng.SLABS}
    assert len(st) == 10
    st.update({name: eng.read(name) for name in ("sum_tree", "min_tree")})
    return st, dict(eng.counters())


def _assert_same(x, y):
    """The ten slabs, both trees and every counter bitwise.  The two loss
    scalars among the counters are the exception, here as in
    test_gpu_multistep.py: they accumulate through cross-workgroup fp32
    atomics, whose order is not fixed, so two runs of one engine differ in
    their last bits (measured here: 4.5470433 against 4.5470428); they are
    held to that file's rel 1e-5."""
    (sx, cx), (sy, cy) = _snapshot(x), _snapshot(y)
    for name in sx:
        assert torch.equal(sx[name], sy[name]), name
    assert cx.keys() == cy.keys()
    for k in cx:
        if k in LOSSES:
            assert cx[k] == pytest.approx(cy[k], rel=1e-5), k
        else:
            assert cx[k] == cy[k], k


def test_destroy_with_everything_live():
    """An engine holding all four pools and all four graphs dies between
    its neighbours' construction and their first step."""
    a = _engine(3, 300)                 # row-block: a training graph exists
    assert not a.info()["persistent"]
    a.train_steps(8, steps_per_graph=4)
    _alloc(a, "pendulum")
    a.rollout_run(1)
    a.eval_alloc(4)
    a.evaluate(1)
    a.collect_alloc(1)
    a.collect_begin(1)
    a.collect_commit()
    assert a.counters()["adam_t_actor"] == 8
    b, c = _engine(3, 300), _engine(3, 300)
    del a
    gc.collect()
    b.step(4)
    c.step(4)
    _assert_same(b, c)
    d = _engine(3, 300)                 # may reuse what A's pools freed
    d.step(4)
    _assert_same(d, b)


@pytest.mark.parametrize("kind", KINDS)
def test_destroy_with_window_open(kind):
    """The destructor drains the rollout stream before it frees the pools
    the window's episodes read and write."""
    o = _obs(kind)
    never = _engine(o, 64)              # lived before the doomed engine did
    _alloc(never, kind)
    out = _run(never, kind)
    want = never.rollout_last_rows()
    assert len(want[2]) > 0

    b, c = _engine(o, 64), _engine(o, 64)
    doomed = _engine(o, 64)
    assert doomed.info()["persistent"]
    _alloc(doomed, kind)
    doomed.collect_alloc(1)
    doomed.collect_begin(1)
    doomed.step(2)
    assert doomed.collect_pending()
    del doomed
    gc.collect()

    b.step(4)
    c.step(4)
    _assert_same(b, c)

    after = _engine(o, 64)
    _alloc(after, kind)
    assert _run(after, kind) == out
    for g, w in zip(after.rollout_last_rows(), want):
        assert np.array_equal(g, w)


def test_replay_async_without_capture():
    eng = _engine(3, 300)
    with pytest.raises(RuntimeError, match="no graph captured"):
        eng.ext.replay_async(eng.h, 1)
