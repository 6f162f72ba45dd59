"""The pipelined steady-state schedule of the persistent megakernel.

At B <= 64 every step of a multi-step launch but the first runs a schedule
of its own: the previous step's tail crew has sampled its batch and computed
its whole critic forward (c_h1..c_h3, q) and ct_h1 under the policy block,
and the actor_t / actor forwards run inside the critic_target quad phase.
Which workgroup computes a tile, and when, must not change one bit of any
value, and nothing precomputed may cross a launch boundary.

  1. step(5) == 5 x step(1) == step(2) + step(3), bitwise, at shapes with a
     partial last row group, a wide concat/action head, a single column
     tile, and uniform replay
  2. slabs reloaded and the replay ingested into BETWEEN launches
  3. q after a 4-step launch against torch on the stored pre-step state
"""

import numpy as np
import pytest
import torch

import _engine_kit as kit
from _engine_kit import Shape

pytestmark = pytest.mark.gpu

CAP, N = 4096, 1024
BUFFERS = ["sum_tree", "min_tree", "bidx", "pri", "bw", "br", "bd", "ba",
           "bs2", "bs", "m_proj", "q", "p_t", "a2", "a_out", "dlog"]


def _engine(shape, mods, tr):
    eng = kit.engine(shape, mods, tr, capacity=CAP)
    assert eng._persistent
    return eng


def _state(eng):
    return kit.snapshot(eng, BUFFERS)


_assert_same = kit.assert_bitwise


SHAPES = [
    # partial last row group (nb = 2) in the quads and the crew forwards,
    # two column tiles
    Shape(50, 128, 3, 1, 51),
    # concat c.L2 reads the next step's ba at width 6, in_pad != in, the
    # action heads have out = 6
    Shape(64, 256, 17, 6, 51),
    # one column tile: quad members 1-3 own no tile but make every arrival
    Shape(8, 64, 3, 1, 11),
    # uniform replay: the tail crew skips the write-back, no barrier
    Shape(64, 256, 3, 1, 51, prioritized=False),
]


@pytest.mark.parametrize("shape", SHAPES, ids=repr)
def test_multistep_launch_is_bitwise_single_steps(shape):
    mods = kit.modules(shape, seed=shape.B)
    tr = kit.transitions(shape, N, seed=shape.B)
    x, y, z = (_engine(shape, mods, tr) for _ in range(3))
    x.step(5)
    for _ in range(5):
        y.step(1)
    ref = _state(y)
    assert ref[1]["adam_t_critic"] == 5
    _assert_same(_state(x), ref, "step(5) vs 5 x step(1)")
    z.step(2)                               # relaunch at odd parity
    z.step(3)
    _assert_same(_state(z), ref, "step(2)+step(3) vs 5 x step(1)")


def test_nothing_precomputed_crosses_a_launch():
    """Between two launches the critic and actor slabs are replaced and
    fresh rows ingested: a multi-step engine must follow exactly like one
    that launches step by step (which never runs the pipelined schedule)."""
    from d4pg_amd.ops import pack_net
    shape = Shape(64, 128, 5, 2, 51)
    mods = kit.modules(shape, seed=1)
    a2, _, c2, _ = kit.modules(shape, seed=2)    # differently seeded W2 / A2
    assert not torch.equal(pack_net(c2), pack_net(mods[2]))
    tr = kit.transitions(shape, N, seed=1)
    fresh = [torch.from_numpy(t) for t in kit.transitions(shape, 512, seed=99)]
    x, y = _engine(shape, mods, tr), _engine(shape, mods, tr)
    for eng, launches in ((x, ([3], [2])), (y, ([1] * 3, [1] * 2))):
        for n in launches[0]:
            eng.step(n)
        eng.load_slab("critic", pack_net(c2))
        eng.load_slab("actor", pack_net(a2))
        eng.ingest(*fresh)
        for n in launches[1]:
            eng.step(n)
    ref = _state(y)
    assert ref[1]["size"] == N + 512
    _assert_same(_state(x), ref, "step(3)|reload|step(2) vs single steps")


def test_q_after_multistep_launch_is_the_last_steps_own():
    """q of the last step of step(4) was computed one step early, by the
    tail crew of step 3: it must come from the critic weights as they stood
    after step 3's Adam and from step 4's own batch.  The pre-step weights
    come from a twin engine stepped 3 times; tolerance is the one-step
    forward's fp32 bound (test_gpu_engine.py: 2e-5)."""
    from d4pg_amd.models import critic
    from d4pg_amd.ops import unpack_net
    shape = Shape(64, 128, 3, 1, 51)
    mods = kit.modules(shape, seed=4)
    tr = kit.transitions(shape, N, seed=4)
    eng, twin = _engine(shape, mods, tr), _engine(shape, mods, tr)
    eng.step(4)
    twin.step(3)
    c = critic(shape.O, shape.A, shape.dist, hidden=shape.H)
    unpack_net(c, twin.store_slab("critic"))
    idx = eng.read("bidx").numpy()
    bs, ba = eng.read("bs"), eng.read("ba")
    assert np.array_equal(bs.numpy(), tr[0][idx])
    assert np.array_equal(ba.numpy(), tr[1][idx])
    with torch.no_grad():
        want = c(bs, ba).numpy()
    got = eng.read("q").numpy()
    print(f"max |q - torch| = {np.abs(got - want).max():.3g}")
    np.testing.assert_allclose(got, want, atol=2e-5)
    # and it is not the previous step's q (which the twin still holds)
    assert np.abs(got - twin.read("q").numpy()).max() > 1e-4
