"""Fence-free quad and crew hand-offs of the persistent megakernel.

Inside a phase the workgroups of a quad (and of the two crews) pass
activations through q_bar / t_bar, which carry no cache fence: producers
store write-through, consumers load past L1.  A missed load of that kind
reads whatever line the CU's L1 still holds; a missed store is seen late or
never.  Two nets:

  1. one persistent step against the row-block path's four step_part
     launches, which hand nothing off inside a launch
  2. a 12-step launch next to a second stream that keeps the memory system
     busy, bitwise against 12 quiet one-step launches

Shapes: the smallest at which a hand-off can go wrong.
"""

import numpy as np
import pytest
import torch

import _engine_kit as kit
from _engine_kit import PARAMS, Shape

pytestmark = pytest.mark.gpu

CAP, N = 4096, 1024
# intermediates both paths write and read() exposes
INTERMEDIATES = ["q", "a_out", "pri", "a2", "p_t", "m_proj", "dlog", "pq"]
BATCH = ["bidx", "bs", "bs2", "ba", "br", "bd", "bw"]


def _engine(shape, mods, tr):
    eng = kit.engine(shape, mods, tr, capacity=CAP)
    assert eng._persistent
    return eng


SHAPES = [
    # one column tile, two quads, crews mostly idle
    Shape(8, 64, 3, 1, 11),
    # partial last row group; 24-byte a2 / a_out / adz rows, so several
    # quads share one 128-B line
    Shape(50, 128, 17, 6, 51),
    # the flagship geometry; 204-byte rows not line-aligned
    Shape(64, 256, 3, 1, 51),
    # the same without trees
    Shape(64, 256, 3, 1, 51, prioritized=False),
]


# Where the commit BEFORE the fence-free hand-offs already exceeded rtol 1e-6 /
# atol 1e-7 against the row-block path: its measured max |difference| per
# array (PARITY.md, "Fence-free hand-offs").  One element of the slab misses
# the bound there — a small weight whose first Adam step (|step| = lr = 1e-4)
# rounds differently in the two Adam spellings.  Those arrays are bounded at
# twice this figure; it was never taken from the build under test.
PARENT_MAX_ABS = {
    ("B50-H128-O17-A6-K51", "slab:actor"): 1.574e-07,
    ("B50-H128-O17-A6-K51", "slab:critic"): 1.658e-07,
    ("B64-H256-O3-A1-K51", "slab:critic"): 1.828e-07,
    ("B64-H256-O3-A1-K51-uniform", "slab:critic"): 1.828e-07,
}


@pytest.mark.parametrize("shape", SHAPES, ids=repr)
def test_persistent_step_matches_handoff_free_rowblock(shape):
    """step(1) on the persistent path against the four step_part masks on
    the row-block path (one wave per row through a whole net: no data
    crosses workgroups inside a launch).  Same seed, slabs and replay, so
    both draw the same batch.  Bound: the one of
    test_gpu_dist.py::test_split_step_matches_full_step, rtol 1e-6 / atol
    1e-7 — the two paths' Adam spellings differ in FMA rounding, nothing
    else may — except the arrays of PARENT_MAX_ABS."""
    mods = kit.modules(shape, seed=shape.B)
    tr = kit.transitions(shape, N, seed=shape.B)
    e1, e2 = _engine(shape, mods, tr), _engine(shape, mods, tr)
    e1.step(1)
    for mask in (e2.PH_CRITIC_GRADS, e2.PH_CRITIC_APPLY, e2.PH_ACTOR_GRADS,
                 e2.PH_ACTOR_APPLY):
        e2.step_part(mask)
    for n in BATCH:
        assert np.array_equal(e1.read(n).numpy(), e2.read(n).numpy()), \
            f"{n}: the two paths drew different batches"
    got = {"slab:" + n: e1.store_slab(n).numpy() for n in PARAMS}
    want = {"slab:" + n: e2.store_slab(n).numpy() for n in PARAMS}
    got.update({n: e1.read(n).numpy() for n in INTERMEDIATES})
    want.update({n: e2.read(n).numpy() for n in INTERMEDIATES})
    for k in got:                    # every figure before any assertion
        d = np.abs(got[k] - want[k])
        rel = d / np.maximum(np.abs(want[k]), 1e-30)
        print(f"{shape!r} {k:20s} max abs {d.max():.3e}  max rel "
              f"{rel[d > 1e-7].max() if (d > 1e-7).any() else 0.0:.3e}")
    for k in got:
        parent = PARENT_MAX_ABS.get((repr(shape), k))
        if parent is None:
            np.testing.assert_allclose(got[k], want[k], rtol=1e-6,
                                       atol=1e-7, err_msg=f"{k} diverged")
        else:
            assert np.abs(got[k] - want[k]).max() <= 2 * parent, \
                f"{k} diverged beyond twice the parent's {parent:.3e}"


def _state(eng):
    return kit.snapshot(
        eng, ["sum_tree", "min_tree", "q", "a_out", "pri"] + BATCH)[0]


@pytest.mark.parametrize("shape", SHAPES, ids=repr)
def test_multistep_launch_under_uneven_load_is_bitwise(shape):
    """A 12-step launch (steady-state steps of both bs parities) runs while
    a second stream copies a 256 MB tensor back and forth, so workgroups of
    one quad see very different memory latencies and arrive far apart.  It
    must equal 12 quiet one-step launches bit for bit.  The side stream
    depends on nothing of the engine's, so the co-resident grid is still
    admitted."""
    mods = kit.modules(shape, seed=shape.B + 1)
    tr = kit.transitions(shape, N, seed=shape.B + 1)
    x, y = _engine(shape, mods, tr), _engine(shape, mods, tr)
    for _ in range(12):
        y.step(1)
    ref = _state(y)
    assert ref["cnt:adam_t_critic"] == 12

    side = torch.cuda.Stream()
    a = torch.empty(64 << 20, dtype=torch.float32, device="cuda")
    b = torch.empty_like(a)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(8):           # ~0.1 ms a copy: outlasts the launch
            b.copy_(a, non_blocking=True)
            a.copy_(b, non_blocking=True)
    x.step(12)
    side.synchronize()
    torch.cuda.synchronize()
    got = _state(x)
    for k in ref:
        assert np.array_equal(got[k], ref[k]), f"{shape!r}: {k} differs"
