"""Multi-step launches of the persistent megakernel — the mode bench.py
measures — against single-step launches (bitwise) and against three eager
torch steps (tolerance).

For B <= 256, step(n) is ONE k_step_persistent launch looping n steps in
the kernel.  What runs only for s > 0 differs by batch size:
  B <= 64        the 32-workgroup tail crew writes PER back, pre-samples
                 step s+1 into the other bs parity buffer and runs the ct/c
                 L1 forwards under the policy megachain      (B = 48, 64)
  64 < B <= 96   the pre-sample runs under the actor Adam    (B = 80)
  96 < B <= 256  every step re-samples in its first phase    (B = 128)
"""

import numpy as np
import pytest

import _engine_kit as kit

pytestmark = pytest.mark.gpu

O, A, H, K = 5, 2, 128, 51
V_MIN, V_MAX = -300.0, 0.0
GAMMA_N = 0.99 ** 5
TAU, LR = 0.001, 1e-4
N = 512
BUFFERS = ["sum_tree", "min_tree", "bidx", "pri", "bw", "br", "bd", "ba",
           "bs2", "m_proj", "q"]


def _shape(B):
    return kit.Shape(B, H, O, A, K)


def _modules(seed=0):
    return kit.modules(_shape(0), seed)


def _transitions(seed=0):
    return kit.transitions(_shape(0), N, seed)


def _engine(B, mods, tr, seed=13):
    return kit.engine(_shape(B), mods, tr, capacity=N, seed=seed)


def _state(eng):
    return kit.snapshot(eng, BUFFERS)


_assert_same = kit.assert_bitwise
_assert_bs_is_gathered = kit.assert_bs_is_gathered


def Eager(mods):
    return kit.Eager(mods, LR, TAU,
                     head=kit.CategoricalHead(V_MIN, V_MAX, GAMMA_N, K))


# ---------------------------------------------------------------------------

@pytest.mark.parametrize("B", [48, 64, 80, 128])
def test_multistep_launch_matches_single_steps(B):
    mods, tr = _modules(seed=B), _transitions(seed=B)
    x, y, z = (_engine(B, mods, tr) for _ in range(3))
    assert x._persistent

    x.step(5)                               # one 5-step launch
    _assert_bs_is_gathered(x, "step(5)")

    eager = Eager(mods)
    eager3 = None
    for i in range(5):                      # five 1-step launches
        y.step(1)
        _assert_bs_is_gathered(y, f"step(1) #{i + 1}")   # odd and even
        if i < 3:
            idx = y.read("bidx").numpy()
            eager.step(*[t[idx] for t in tr])
            if i == 2:
                eager3 = eager.slabs()
                y3 = {n: y.store_slab(n).numpy() for n in eager3}
    ref = _state(y)
    _assert_same(_state(x), ref, "step(5) vs 5 x step(1)")

    z.step(2)                               # relaunch at odd parity
    _assert_bs_is_gathered(z, "step(2)")
    z.step(3)
    _assert_bs_is_gathered(z, "step(2)+step(3)")
    _assert_same(_state(z), ref, "step(2)+step(3) vs 5 x step(1)")

    # ---- three-step oracle: Adam bias correction at t > 1, compounded
    # soft updates.  Single-step tolerance is 2e-5; Adam bounds a step's
    # parameter drift by lr, so three steps get 3x that.  v is quadratic
    # in the gradient and spans many decades, so it is also held to 1e-4
    # of the slab's largest entry; so is m (max |m| is ~5e-3, where the
    # absolute 6e-5 alone would pass a 1% error).
    for n in eager3:
        err = np.abs(y3[n] - eager3[n]).max()
        scale = np.abs(eager3[n]).max()
        print(f"B={B} {n}: max abs err {err:.3g} (max |ref| {scale:.3g})")
    for n in eager3:
        np.testing.assert_allclose(y3[n], eager3[n], atol=6e-5, err_msg=n)
    for n in ("m_actor", "m_critic", "v_actor", "v_critic"):
        scale = np.abs(eager3[n]).max()
        assert np.abs(y3[n] - eager3[n]).max() <= 1e-4 * scale, n


def test_wide_odd_batch_gradients_match_eager():
    """B=640 takes the per-layer MFMA path with a batch that is no
    power-of-two multiple of the split-K chunk (20 chunks of 32 rows over
    16 segments): the empty tail segments of k_mfma_dw must contribute
    zero to BOTH nets' dW.  Tolerance: the wide path's 1e-4
    (test_gpu_wide.py)."""
    B = 640
    mods, tr = _modules(seed=B), _transitions(seed=B)
    eng = _engine(B, mods, tr)
    assert not eng._persistent
    eng.step(1)
    idx = eng.read("bidx").numpy()
    eager = Eager(mods)
    eager.step(*[t[idx] for t in tr])
    for n, want in eager.grads().items():
        got = eng.store_slab(n).numpy()
        print(f"B={B} {n}: max abs err {np.abs(got - want).max():.3g} "
              f"(max |ref| {np.abs(want).max():.3g})")
        np.testing.assert_allclose(got, want, atol=1e-4, err_msg=n)
        # and relative to the slab: the worst-case fp32 error of a 640-term
        # sum is 640 * 2^-24 ~ 4e-5 of the summed magnitudes; 1e-3 of the
        # largest entry leaves 25x for cancellation and the layer chain,
        # while a stale split-K partial shows up at order 1
        assert np.abs(got - want).max() <= 1e-3 * np.abs(want).max(), n


def test_graph_replay_matches_uncaptured_rowblock():
    """B=300 is past the persistent path, so train_steps really captures
    and replays a hipGraph: two replays of a 3-step graph == step(6)."""
    B = 300
    mods, tr = _modules(seed=B), _transitions(seed=B)
    x, y = _engine(B, mods, tr), _engine(B, mods, tr)
    assert not x._persistent
    x.step(6)
    y.train_steps(6, steps_per_graph=3)
    assert y._captured == 3
    _assert_same(_state(x), _state(y), "step(6) vs graph 2 x 3")
    assert x.counters()["adam_t_critic"] == 6
