"""Exact checks of the replay's write side: Engine::ingest on both of its
paths (the one-workgroup k_replay_add up to 4096 rows, k_replay_copy plus the
k_tree_build_level sweep above that) and synth_fill, against the plain numpy
ring in tests/_oracles.py.

After every ingest call the whole device replay (rows [0, size), size, pos
and both trees over their full 2*tree_cap arrays) is compared with the
oracle.  Rows, counters and the trees over unit leaves are compared for
EQUALITY.  A leaf that is a computed power is compared at 2 ulp of a double
(HIP documents pow at 1 ulp, the host's is under 1 ulp), after which both
trees must be bitwise what build_trees gives over the device's own leaves.
"""

import numpy as np
import pytest
import torch

import _engine_kit as kit
import _oracles as orc

pytestmark = pytest.mark.gpu

# obs != act and both odd/even mixed, so an obs/act index mix-up shows
O, A, H, K, B = 5, 2, 64, 51, 64
V_MIN, V_MAX = -300.0, 0.0
DIST = {"type": "categorical", "v_min": V_MIN, "v_max": V_MAX, "n_atoms": K}
ALPHA = np.float64(np.float32(0.6))     # the engine holds per_alpha as float


def _engine(capacity, seed=3):
    return kit.engine(kit.Shape(B, H, O, A, K), capacity=capacity, seed=seed)


def _rows(rng, T):
    """T fresh random transitions: every call's rows differ from every
    other's, so a stale or mixed-up row cannot compare equal."""
    return kit.draw_rows(rng, O, A, T, p_done=0.3)


def _ingest(eng, rows):
    eng.ingest(*[torch.from_numpy(np.ascontiguousarray(x)) for x in rows])


def _state(eng):
    st = eng.ext.replay_state(eng.h)
    out = {k: st[k].numpy() for k in ("s", "a", "s2", "sum_tree", "min_tree")}
    out["r"] = st["r"].numpy().ravel()
    out["d"] = st["d"].numpy().ravel()
    out["size"], out["pos"] = int(st["size"]), int(st["pos"])
    return out


def _leaf(p):
    """The leaf of a new row at max_priority p, in float64."""
    return np.float64(np.float32(p)) ** ALPHA


def _within_2ulp(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want) <= 2 * np.spacing(want)


def _check(eng, ring, exact=True):
    """Device replay == oracle.  exact: every oracle leaf is exactly
    representable (1.0 or injected), so the trees are compared bitwise with
    the oracle's.  Otherwise the two-stage comparison of the module
    docstring."""
    st = _state(eng)
    cap = ring.tree_cap
    assert (st["size"], st["pos"]) == (ring.size, ring.pos)
    for name, want in zip(("s", "a", "r", "s2", "d"), ring.occupied()):
        assert np.array_equal(st[name], want), name
    assert st["sum_tree"].shape == st["min_tree"].shape == (2 * cap,)
    if exact:
        want_s, want_m = ring.trees()
    else:
        leaves = st["sum_tree"][cap:cap + ring.size]
        assert np.array_equal(st["min_tree"][cap:cap + ring.size], leaves)
        assert _within_2ulp(leaves, ring.leaves[:ring.size]).all()
        want_s, want_m = orc.build_trees(leaves, cap)
    assert np.array_equal(st["sum_tree"], want_s)
    assert np.array_equal(st["min_tree"], want_m)
    return st


def _same_state(x, y):
    return all(np.array_equal(x[k], y[k]) for k in x)


# ---------------------------------------------------------------------------
# the one-workgroup path across the ring's end
# ---------------------------------------------------------------------------

# The third call ends exactly at capacity (pos -> 0), a single row follows,
# and the last call spans the wrap and overwrites all but one slot.
@pytest.mark.parametrize("capacity,calls", [
    (600, [300, 250, 50, 1, 100, 599]),     # tree_cap 1024 > capacity
    (512, [256, 200, 56, 1, 100, 511]),     # tree_cap == capacity
])
def test_small_path_wrap(capacity, calls):
    eng = _engine(capacity)
    cap = eng.info()["tree_cap"]
    assert cap == (1024 if capacity == 600 else 512)
    ring = orc.RingOracle(capacity, cap)
    rng = np.random.default_rng(capacity)
    for n, T in enumerate(calls):
        rows = _rows(rng, T)
        _ingest(eng, rows)
        ring.add(*rows)
        st = _check(eng, ring)
        if n == 2:
            assert st["pos"] == 0 and st["size"] == capacity
    assert ring.pos == sum(calls) % capacity
    assert st["sum_tree"][1] == capacity


# ---------------------------------------------------------------------------
# T = 4096 | 4097: the path switch, and the bulk path across the ring's end
# ---------------------------------------------------------------------------

def test_path_switch_and_bulk_wrap():
    capacity, calls = 5000, [4096, 4097, 4097]
    rng = np.random.default_rng(5)
    data = [_rows(rng, T) for T in calls]
    eng = _engine(capacity)
    cap = eng.info()["tree_cap"]
    assert cap == 8192
    ring = orc.RingOracle(capacity, cap)
    for rows in data:
        _ingest(eng, rows)
        ring.add(*rows)
        _check(eng, ring)
    assert ring.pos == sum(calls) % capacity and ring.size == capacity
    big = _state(eng)

    # the same rows through the one-workgroup path only
    eng2 = _engine(capacity)
    flat = [np.concatenate([d[i] for d in data]) for i in range(5)]
    for lo in range(0, sum(calls), 1000):
        _ingest(eng2, [x[lo:lo + 1000] for x in flat])
    assert _same_state(big, _state(eng2))


# ---------------------------------------------------------------------------
# the leaf of a new row when max_priority != 1
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("p", [1e-3, 2.5])
def test_new_row_priority(p):
    capacity = 8192
    eng = _engine(capacity)
    cap = eng.info()["tree_cap"]
    ring = orc.RingOracle(capacity, cap)
    eng.set_schedule(0, max_priority=p)
    rng = np.random.default_rng(8)
    for T in (100, 4097):               # device pow, then host pow
        rows = _rows(rng, T)
        _ingest(eng, rows)
        ring.add(*rows, leaf=_leaf(p))
        st = _check(eng, ring, exact=False)
    leaves = st["sum_tree"][cap:cap + 4197]
    small, bulk = np.unique(leaves[:100]), np.unique(leaves[100:])
    assert len(small) == 1 and len(bulk) == 1
    ulps = (small[0] - bulk[0]) / np.spacing(bulk[0])
    print(f"p={p}: small-path leaf {small[0]!r}, bulk-path leaf {bulk[0]!r}, "
          f"oracle {_leaf(p)!r}; small - bulk = {ulps:+.0f} ulp")
    assert st["sum_tree"][1] == pytest.approx(4197 * _leaf(p), rel=1e-12)
    assert eng.counters()["max_priority"] == float(np.float32(p))


# ---------------------------------------------------------------------------
# ingest over an injected non-uniform tree: the overwritten minimum
# ---------------------------------------------------------------------------

def test_ingest_over_nonuniform_tree_moves_minimum():
    capacity = 512
    eng = _engine(capacity)
    cap = eng.info()["tree_cap"]
    rng = np.random.default_rng(12)
    rp = dict(zip(("s", "a", "r", "s2", "d"), _rows(rng, capacity)))
    leaves = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), capacity))
    k = int(np.argmin(leaves))
    assert 0 < k < capacity - 40            # the 40-row call does not wrap
    st0, mt0 = orc.build_trees(leaves, cap)
    eng.ext.load_replay_state(
        eng.h, *[torch.from_numpy(rp[n]) for n in ("s", "a", "r", "s2", "d")],
        torch.from_numpy(st0), torch.from_numpy(mt0), capacity, k, 1.0)
    ring = orc.RingOracle(capacity, cap)
    ring.rows = {n: v.copy() for n, v in rp.items()}
    ring.leaves = leaves.copy()
    ring.size, ring.pos = capacity, k
    _check(eng, ring)                       # the injection round-trips
    assert mt0[1] == leaves[k]

    for T in (1, 40):
        rows = _rows(rng, T)
        _ingest(eng, rows)
        ring.add(*rows)                     # max_priority 1: leaf exactly 1
        st = _check(eng, ring)
        assert st["min_tree"][1] == ring.leaves.min() > leaves[k]
    assert (st["sum_tree"][cap + k:cap + k + 41] == 1.0).all()
    assert ring.pos == k + 41


# ---------------------------------------------------------------------------
# ingest after training has raised max_priority on the device
# ---------------------------------------------------------------------------

# A priority is <m, q> + per_eps with m and q both distributions, so it never
# exceeds 1 and a fresh engine's max_priority stays 1.0 through training.
# Starting the run at 1e-3 lets the steps raise it (an untrained critic's q is
# near uniform, <m, q> about 1/51), so the new rows' leaf is a device pow of a
# value the device itself produced.
@pytest.mark.parametrize("mp0", [1.0, 1e-3])
def test_ingest_after_training(mp0):
    import copy
    from d4pg_amd.models import actor, critic
    capacity = 600
    eng = _engine(capacity)
    cap = eng.info()["tree_cap"]
    torch.manual_seed(0)
    a, c = actor(O, A, hidden=H), critic(O, A, DIST, hidden=H)
    eng.load_from_modules(a, copy.deepcopy(a), c, copy.deepcopy(c))
    eng.set_schedule(0, max_priority=mp0)
    ring = orc.RingOracle(capacity, cap)
    rng = np.random.default_rng(2)
    rows = _rows(rng, 512)
    _ingest(eng, rows)
    ring.add(*rows, leaf=_leaf(mp0))
    _check(eng, ring, exact=(mp0 == 1.0))
    eng.step(3)
    mp = eng.counters()["max_priority"]
    print(f"max_priority {mp0!r} -> {mp!r} after 3 steps")
    if mp0 == 1.0:
        assert mp == 1.0
    else:
        pri = eng.read("pri").numpy()
        assert float(np.float32(mp0)) < pri.max() <= mp < 1.0
    before = _state(eng)

    rows = _rows(rng, 10)
    _ingest(eng, rows)
    ring.add(*rows, leaf=_leaf(mp))
    st = _state(eng)
    assert (st["size"], st["pos"]) == (522, 522)
    for name, want in zip(("s", "a", "r", "s2", "d"), ring.occupied()):
        assert np.array_equal(st[name], want), name
    new = st["sum_tree"][cap + 512:cap + 522]
    assert _within_2ulp(new, _leaf(mp)).all()
    assert np.array_equal(st["min_tree"][cap + 512:cap + 522], new)
    # trained leaves are untouched, the rest of the range is still empty
    assert np.array_equal(st["sum_tree"][cap:cap + 512],
                          before["sum_tree"][cap:cap + 512])
    assert np.array_equal(st["min_tree"][cap:cap + 512],
                          before["min_tree"][cap:cap + 512])
    assert (st["sum_tree"][cap + 522:] == 0).all()
    assert np.isinf(st["min_tree"][cap + 522:]).all()
    n = np.arange(1, cap)
    assert np.array_equal(st["sum_tree"][n],
                          st["sum_tree"][2 * n] + st["sum_tree"][2 * n + 1])
    assert np.array_equal(st["min_tree"][n],
                          np.minimum(st["min_tree"][2 * n],
                                     st["min_tree"][2 * n + 1]))


# ---------------------------------------------------------------------------
# one call longer than the ring
# ---------------------------------------------------------------------------

# Rows t and t + capacity of one call map to the same slot; the slot must end
# up holding ONE whole transition, the last one mapped to it.  300 and 3000
# keep no more rows than the one-workgroup path takes; 4500 keeps 4500 and
# stays on the bulk path.  A first short call moves pos off 0.
@pytest.mark.parametrize("capacity,T", [(300, 700), (3000, 7000),
                                        (4500, 10000)])
def test_one_call_longer_than_the_ring(capacity, T):
    eng = _engine(capacity)
    cap = eng.info()["tree_cap"]
    ring = orc.RingOracle(capacity, cap)
    rng = np.random.default_rng(T)
    for n in (50, T):
        rows = _rows(rng, n)
        _ingest(eng, rows)
        ring.add(*rows)
        _check(eng, ring)
    assert ring.pos == (50 + T) % capacity and ring.size == capacity
    # each slot holds the last row of the long call mapped to it
    slot = (50 + np.arange(T)) % capacity
    assert np.array_equal(ring.rows["r"][slot[-capacity:]],
                          rows[2][-capacity:])


# ---------------------------------------------------------------------------
# synth_fill
# ---------------------------------------------------------------------------

def test_synth_fill_tree():
    eng = _engine(1000)
    cap = eng.info()["tree_cap"]
    assert cap == 1024
    eng.synth_fill(777, seed=5)
    st = _state(eng)
    assert (st["size"], st["pos"]) == (777, 777)
    want_s, want_m = orc.build_trees(np.ones(777), cap)
    assert np.array_equal(st["sum_tree"], want_s)
    assert np.array_equal(st["min_tree"], want_m)
    assert st["s"].shape == (777, O) and st["a"].shape == (777, A)
    assert np.abs(st["s"]).max() <= 1 and np.abs(st["a"]).max() <= 1
    assert len(np.unique(st["r"])) > 700 and (st["r"] <= 0).all()
