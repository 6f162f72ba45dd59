"""The shared kit of the GPU engine tests (tests/_engine_kit.py), on the CPU:
the bitwise comparator really is one, the slab packer has the engine's layout,
and the input builders are deterministic in their seed."""

import copy

import numpy as np
import pytest
import torch

import _engine_kit as kit
from d4pg_amd.ops import pack_net

BUFFERS = ["q", "bidx"]


class StubEngine:
    """store_slab / read / counters over plain arrays."""

    def __init__(self):
        rng = np.random.default_rng(0)
        self.slabs = {n: rng.standard_normal(7).astype("f") for n in kit.SLABS}
        self.bufs = {"q": rng.random((4, 3)).astype("f"),
                     "bidx": np.arange(4, dtype=np.int64)}
        self.cnt = dict({n: 5 for n in kit.INT_COUNTERS}, loss_critic=1.25,
                        loss_actor=-40.0)

    def store_slab(self, n):
        return torch.from_numpy(self.slabs[n].copy())

    def read(self, n):
        return torch.from_numpy(self.bufs[n].copy())

    def counters(self):
        return dict(self.cnt)


def _differs(change):
    x, y = StubEngine(), StubEngine()
    change(y)
    with pytest.raises(AssertionError):
        kit.assert_bitwise(kit.snapshot(x, BUFFERS), kit.snapshot(y, BUFFERS),
                           "stub")


def _last_bit(a, i):
    a.view(np.uint32)[i] ^= 1


def test_equal_snapshots_pass():
    st, cnt = kit.snapshot(StubEngine(), BUFFERS)
    assert set(st) == ({"slab:" + n for n in kit.SLABS} | set(BUFFERS)
                       | {"cnt:" + n for n in kit.INT_COUNTERS})
    assert len(kit.SLABS) == 10 and kit.SLABS[:4] == kit.PARAMS
    kit.assert_bitwise((st, cnt), kit.snapshot(StubEngine(), BUFFERS), "stub")


def test_one_differing_value_fails():
    _differs(lambda e: _last_bit(e.slabs["v_critic"], 3))
    _differs(lambda e: _last_bit(e.bufs["q"].reshape(-1), 5))
    _differs(lambda e: e.cnt.update(rng_epoch=6))
    _differs(lambda e: e.cnt.update(loss_critic=1.25 * (1 + 1e-3)))
    _differs(lambda e: e.cnt.update(loss_actor=-40.0 * (1 + 1e-3)))


def test_loss_scalars_are_approximate():
    x, y = StubEngine(), StubEngine()
    y.cnt.update(loss_critic=1.25 * (1 + 1e-6), loss_actor=-40.0 * (1 - 1e-6))
    kit.assert_bitwise(kit.snapshot(x, BUFFERS), kit.snapshot(y, BUFFERS),
                       "stub")


def test_a_key_on_one_side_only_fails():
    x = StubEngine()
    full, part = kit.snapshot(x, BUFFERS), kit.snapshot(x, ["q"])
    for a, b in ((full, part), (part, full)):
        with pytest.raises(AssertionError):
            kit.assert_bitwise(a, b, "stub")


SHAPE = kit.Shape(4, 8, 5, 2, 11)


def test_pack_has_the_engine_layout():
    a, _, c, _ = kit.modules(SHAPE, seed=1)
    for m in (a, c):
        assert np.array_equal(kit.pack(m), pack_net(m).numpy())
        out = m(*[torch.ones(3, n) for n in ((5,) if m is a else (5, 2))])
        (out ** 2).sum().backward()     # (a softmax row's plain sum is 1)
        want = np.concatenate(
            [np.concatenate([getattr(m, n).weight.grad.numpy().T.reshape(-1),
                             getattr(m, n).bias.grad.numpy()])
             for n in ["fc1", "fc2", "fc2_2", "fc3"]])
        got = kit.pack(m, lambda p: p.grad)
        assert got.shape == kit.pack(m).shape and np.array_equal(got, want)
        assert np.abs(got).max() > 0


def test_shape_ids_and_paths():
    assert repr(kit.Shape(50, 128, 17, 6, 51)) == "B50-H128-O17-A6-K51"
    assert repr(kit.Shape(64, 256, 3, 1, 51, prioritized=False)) == \
        "B64-H256-O3-A1-K51-uniform"
    assert repr(kit.Shape(520, 100, 3, 1, 51, precision="bf16")) == \
        "B520-H100-O3-A1-K51-bf16"
    assert [kit.Shape(b, 8, 3, 1, 11).path for b in (256, 257, 512, 513)] == \
        ["persistent", "rowblock", "rowblock", "wide"]


def _bytes(mods):
    return [v.numpy().tobytes() for m in mods for v in m.state_dict().values()]


def test_builders_are_deterministic_in_the_seed():
    mods = kit.modules(SHAPE, seed=3)
    assert _bytes(mods) == _bytes(kit.modules(SHAPE, seed=3))
    assert _bytes(mods) != _bytes(kit.modules(SHAPE, seed=4))
    assert _bytes(mods[:1]) == _bytes(mods[1:2])        # targets are copies
    assert mods[0] is not mods[1] and mods[2] is not mods[3]
    tr = kit.transitions(SHAPE, 16, seed=3)
    assert [x.shape for x in tr] == [(16, 5), (16, 2), (16,), (16, 5), (16,)]
    again, other = (kit.transitions(SHAPE, 16, seed=s) for s in (3, 4))
    assert [x.tobytes() for x in tr] == [x.tobytes() for x in again]
    assert all(x.tobytes() != y.tobytes() for x, y in zip(tr[:4], other[:4]))
    q = copy.copy(SHAPE)
    q.head = "quantile"
    assert q.dist == {"type": "quantile", "n_atoms": 11, "kappa": 1.0}
