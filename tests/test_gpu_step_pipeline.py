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

import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

V_MIN, V_MAX = -300.0, 0.0
GAMMA_N = 0.99 ** 5
TAU, LR = 0.001, 1e-4
CAP, N = 4096, 1024
SLABS = ["actor", "actor_target", "critic", "critic_target", "g_actor",
         "g_critic", "m_actor", "v_actor", "m_critic", "v_critic"]
BUFFERS = ["sum_tree", "min_tree", "bidx", "pri", "bw", "br", "bd", "ba",
           "bs2", "bs", "m_proj", "q", "p_t", "a2", "a_out", "dlog"]
INT_COUNTERS = ["beta_t", "adam_t_actor", "adam_t_critic", "rng_epoch",
                "size", "pos"]


class Shape:
    def __init__(self, B, H, O, A, K, prioritized=True):
        self.B, self.H, self.O, self.A, self.K = B, H, O, A, K
        self.prioritized = prioritized
        self.dist = {"type": "categorical", "v_min": V_MIN, "v_max": V_MAX,
                     "n_atoms": K}

    def __repr__(self):
        return (f"B{self.B}-H{self.H}-O{self.O}-A{self.A}-K{self.K}"
                + ("" if self.prioritized else "-uniform"))

    def modules(self, seed):
        from d4pg_amd.models import actor, critic
        torch.manual_seed(seed)
        a = actor(self.O, self.A, hidden=self.H)
        c = critic(self.O, self.A, self.dist, hidden=self.H)
        return a, copy.deepcopy(a), c, copy.deepcopy(c)

    def transitions(self, n, seed):
        rng = np.random.default_rng(seed)
        return (rng.standard_normal((n, self.O)).astype("f"),
                rng.uniform(-1, 1, (n, self.A)).astype("f"),
                rng.uniform(-30, 0, n).astype("f"),
                rng.standard_normal((n, self.O)).astype("f"),
                (rng.random(n) < 0.05).astype("f"))

    def engine(self, mods, tr, seed=13):
        from d4pg_amd.ops import FusedEngine
        eng = FusedEngine(obs_dim=self.O, act_dim=self.A, hidden=self.H,
                          n_atoms=self.K, batch=self.B, capacity=CAP,
                          v_min=V_MIN, v_max=V_MAX, gamma_n=GAMMA_N, tau=TAU,
                          lr_actor=LR, lr_critic=LR, seed=seed,
                          prioritized=self.prioritized)
        eng.load_from_modules(*mods)
        eng.ingest(*[torch.from_numpy(x) for x in tr])
        assert eng._persistent
        return eng


def _state(eng):
    st = {"slab:" + n: eng.store_slab(n).numpy() for n in SLABS}
    st.update({n: eng.read(n).numpy() for n in BUFFERS})
    cnt = eng.counters()
    st.update({"cnt:" + n: cnt[n] for n in INT_COUNTERS})
    return st, cnt


def _assert_same(x, y, what):
    sx, cx = x
    sy, cy = y
    for k in sx:
        assert np.array_equal(sx[k], sy[k]), f"{what}: {k} differs"
    # the loss scalars accumulate through cross-workgroup fp32 atomics,
    # whose order is not fixed: approximately equal only
    for k in ("loss_critic", "loss_actor"):
        assert cx[k] == pytest.approx(cy[k], rel=1e-5), f"{what}: {k}"


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
    mods = shape.modules(seed=shape.B)
    tr = shape.transitions(N, seed=shape.B)
    x, y, z = (shape.engine(mods, tr) for _ in range(3))
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
    mods = shape.modules(seed=1)
    a2, _, c2, _ = shape.modules(seed=2)    # differently seeded W2 / A2
    assert not torch.equal(pack_net(c2), pack_net(mods[2]))
    tr = shape.transitions(N, seed=1)
    fresh = [torch.from_numpy(t) for t in shape.transitions(512, seed=99)]
    x, y = shape.engine(mods, tr), shape.engine(mods, tr)
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
    mods = shape.modules(seed=4)
    tr = shape.transitions(N, seed=4)
    eng, twin = shape.engine(mods, tr), shape.engine(mods, tr)
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
