"""Exact checks of the engine's prioritized replay: the leaf every probe
draws, the importance-sampling weights, the is_weighting=True loss path and
the bitwise parent == left + right tree invariant after write-back.

A non-uniform tree is injected with load_replay_state; the probes come from
philox4x32-10(key=seed, ctr_lo=probe, ctr_hi=rng_epoch), so the whole draw
is reproduced on the CPU (tests/_oracles.py) and compared for EQUALITY.
"""

import copy

import numpy as np
import pytest
import torch

import _engine_kit as kit
import _oracles as orc

pytestmark = pytest.mark.gpu

O, A, H, K = 5, 2, 128, 51
V_MIN, V_MAX = -300.0, 0.0
GAMMA_N = 0.99 ** 5
ALPHA = float(np.float32(0.6))          # the engine holds per_alpha as float
BETA0, BETA_ITERS = 0.4, 10
SEED = 21
_inject = kit.inject_replay


def _shape(B=0):
    return kit.Shape(B, H, O, A, K)


def _engine(B, capacity, is_weighting=False):
    return kit.engine(_shape(B), capacity=capacity, seed=SEED,
                      per_beta0=BETA0, per_beta_iters=BETA_ITERS,
                      is_weighting=is_weighting)


def _modules(seed=0):
    return kit.modules(_shape(), seed)


def _replay(size, seed=0):
    return kit.per_replay(_shape(), size, seed)


def test_fresh_engine_tree_fill():
    """What build_trees assumes about unoccupied leaves, and the epoch the
    first step samples with."""
    eng = _engine(64, 512)
    st = eng.ext.replay_state(eng.h)
    want_s, want_m = orc.build_trees([], eng.info()["tree_cap"])
    assert np.array_equal(st["sum_tree"].numpy(), want_s)
    assert np.array_equal(st["min_tree"].numpy(), want_m)
    cnt = eng.counters()
    # counters() reports steps COMPLETED; the device counter is pre-advanced
    # by one, so the first step draws with philox epoch 1
    assert cnt["rng_epoch"] == 0 and cnt["beta_t"] == 0


# capacity 512 -> tree_cap 2^9: the 4-ary walk ends on its odd final level;
# capacity 1024 -> 2^10: it does not.  size < tree_cap leaves the top empty.
@pytest.mark.parametrize("capacity,size", [(512, 300), (1024, 700)])
@pytest.mark.parametrize("B", [64, 300])     # p_sample / k_per_sample
def test_exact_draw_and_is_weights(B, capacity, size):
    eng = _engine(B, capacity)
    eng.load_from_modules(*_modules())
    rp = _replay(size, seed=capacity)
    assert eng.counters()["rng_epoch"] == 0      # fresh: first epoch is 1
    worst = 0.0
    # start, middle and saturated points of the beta schedule
    for steps_done in (0, 5, 50):
        st, mt, cap = _inject(eng, rp)           # the step rewrites leaves
        assert cap == capacity
        eng.set_schedule(steps_done)
        cnt = eng.counters()
        assert cnt["rng_epoch"] == cnt["beta_t"] == steps_done
        epoch = cnt["rng_epoch"] + 1             # completed steps + 1
        eng.step(1)
        want = np.array([
            orc.descend(st, cap, orc.probe_mass(SEED, epoch, i, st[1]), size)
            for i in range(B)])
        idx = eng.read("bidx").numpy()
        assert np.array_equal(idx, want)
        assert idx.max() < size and len(np.unique(idx)) > 8
        bw = eng.read("bw").numpy()
        w = orc.is_weights(st, mt, want, size, BETA0, BETA_ITERS,
                           cnt["beta_t"])
        worst = max(worst, float(np.abs(bw / w - 1).max()))
        np.testing.assert_allclose(bw, w, rtol=1e-5)
        assert bw.max() <= 1 + 1e-6
        assert bw.min() < 0.5                    # genuinely non-uniform
        assert np.array_equal(eng.read("br").numpy(), rp["r"][idx])
    print(f"B={B} cap={capacity}: max rel err of bw = {worst:.3g}")


# Seeds whose first-epoch draw TIES by construction.  On a full tree of
# unit leaves the total is a power of two, so mass = u * N is exact and a
# probe whose float32 u is a multiple of 1/N lands exactly on the boundary
# between leaves j-1 and j (mass == j).  `mass <= left` must send it LEFT,
# to leaf j-1; a `<` descent ends on leaf j.  The lowest set bit of j picks
# the tree level, hence the comparison, that resolves the tie (found by
# scanning seeds with the philox oracle):
#   tree_cap 2^9  (4 four-ary steps + the odd final binary level)
#     j odd -> final level; j = 2 mod 4 -> g0/g2; j = 4 mod 8 -> s01
#   tree_cap 2^12 (6 four-ary steps, no final level)
#     j odd -> g0/g2; j = 2 mod 4 -> s01
TIE_SEEDS = {512: [(1123, 12, 235), (2692, 7, 450), (2226, 50, 236)],
             4096: [(224, 34, 867), (312, 26, 522)]}


@pytest.mark.parametrize("capacity", [512, 4096])
@pytest.mark.parametrize("B", [64, 300])     # p_sample / k_per_sample
def test_tie_goes_left(B, capacity):
    eng = _engine(B, capacity)
    eng.load_from_modules(*_modules())
    rp = _replay(capacity, seed=capacity)
    rp["leaves"] = np.ones(capacity)
    for seed, probe, j in TIE_SEEDS[capacity]:
        st, _, cap = _inject(eng, rp)
        assert cap == capacity and st[1] == capacity
        eng.set_seed(seed)
        eng.set_schedule(0)
        mass = np.array([orc.probe_mass(seed, 1, i, st[1])
                         for i in range(B)])
        ties = np.nonzero((mass == np.floor(mass)) & (mass < capacity))[0]
        assert probe in ties and mass[probe] == j
        eng.step(1)
        idx = eng.read("bidx").numpy()
        want = np.array([orc.descend(st, cap, m, capacity) for m in mass])
        assert np.array_equal(idx, want)
        # left of the boundary, where a strict `<` would have gone right
        assert np.array_equal(idx[ties], mass[ties].astype(np.int64) - 1)


def _eager_weighted_grad(mods, o):
    """g_critic of the IS-weighted CE loss, in the engine's slab layout."""
    from d4pg_amd.algo.projection import categorical_projection
    a, at, c, ct = [copy.deepcopy(m) for m in mods]
    t = {k: torch.from_numpy(v) for k, v in o.items()}
    with torch.no_grad():
        m = categorical_projection(ct(t["bs2"], at(t["bs2"])), t["br"],
                                   t["bd"], V_MIN, V_MAX, GAMMA_N)
    q = c(t["bs"], t["ba"])
    loss = (t["bw"] * -(m * torch.log(q + 1e-10)).sum(1)).mean()
    c.zero_grad()
    loss.backward()
    return torch.cat([torch.cat([getattr(c, n).weight.grad.t().reshape(-1),
                                 getattr(c, n).bias.grad])
                      for n in ["fc1", "fc2", "fc2_2", "fc3"]]).numpy()


# persistent megakernel / row-block / per-layer MFMA path, with the path's
# existing g_critic tolerance
@pytest.mark.parametrize("B,g_atol", [(64, 3e-5), (300, 3e-5), (640, 1e-4)])
def test_is_weighting_scales_loss_and_gradient(B, g_atol):
    mods = _modules(seed=B)
    rp = _replay(700, seed=B)
    out = {}
    for flag in (True, False):
        eng = _engine(B, 1024, is_weighting=flag)
        eng.load_from_modules(*mods)
        _inject(eng, rp)
        eng.step(1)
        o = {n: eng.read(n).numpy() for n in
             ["bs", "ba", "br", "bs2", "bd", "bw", "bidx", "q", "m_proj",
              "dlog"]}
        o["loss"] = eng.counters()["loss_critic"]
        o["g_critic"] = eng.store_slab("g_critic").numpy()
        out[flag] = o
    w, u = out[True], out[False]
    assert np.array_equal(w["bidx"], u["bidx"])      # same draw, same tree
    assert np.array_equal(w["bw"], u["bw"])
    bw = w["bw"].astype(np.float64)
    assert bw.min() < 0.5 and bw.max() <= 1 + 1e-6
    q, m = w["q"].astype(np.float64), w["m_proj"].astype(np.float64)
    np.testing.assert_allclose(w["dlog"], bw[:, None] * (q - m) / B,
                               atol=5e-6)
    np.testing.assert_allclose(u["dlog"], (q - m) / B, atol=5e-6)
    # the unweighted twin must differ, or the above proves nothing
    assert np.abs(w["dlog"] - u["dlog"]).max() > 0.1 * np.abs(u["dlog"]).max()
    ce = -(m * np.log(q + 1e-10)).sum(axis=1)
    assert w["loss"] == pytest.approx(float((bw * ce).mean()), rel=1e-4)
    assert u["loss"] == pytest.approx(float(ce.mean()), rel=1e-4)
    batch = {k: w[k] for k in ["bs", "ba", "br", "bs2", "bd", "bw"]}
    g = _eager_weighted_grad(mods, batch)
    err = np.abs(w["g_critic"] - g).max()
    print(f"B={B}: max|g_critic - eager| = {err:.3g} "
          f"(max|g| = {np.abs(g).max():.3g})")
    np.testing.assert_allclose(w["g_critic"], g, atol=g_atol)
    # and the unweighted twin against the unweighted loss (B=640 is no
    # power-of-two multiple of the split-K chunk: empty dW segments)
    batch["bw"] = np.ones(B, np.float32)
    gu = _eager_weighted_grad(mods, batch)
    print(f"B={B}: unweighted max|g_critic - eager| = "
          f"{np.abs(u['g_critic'] - gu).max():.3g}")
    np.testing.assert_allclose(u["g_critic"], gu, atol=g_atol)
    assert np.abs(w["g_critic"] - u["g_critic"]).max() > 10 * g_atol


# B=640 repairs the tree with k_per_leaves + k_per_level4 (B > 512)
@pytest.mark.parametrize("B", [64, 300, 640])
def test_tree_invariant_after_writeback(B):
    eng = _engine(B, 1024)
    eng.load_from_modules(*_modules(seed=1))
    rp = _replay(700, seed=B + 1)
    st0, _, cap = _inject(eng, rp, max_priority=1e-3)
    drawn, run_max = [], np.float32(1e-3)
    for _ in range(3):
        eng.step(1)
        idx, pri = eng.read("bidx").numpy(), eng.read("pri").numpy()
        drawn.append((idx, pri))
        run_max = max(run_max, pri.max())
    st = eng.read("sum_tree").numpy()
    mt = eng.read("min_tree").numpy()
    n = np.arange(1, cap)
    assert np.array_equal(st[n], st[2 * n] + st[2 * n + 1])
    assert np.array_equal(mt[n], np.minimum(mt[2 * n], mt[2 * n + 1]))
    # leaves drawn exactly once over the three steps carry pri^alpha.  The
    # device pow and the host pow are each within 1 ulp of the true value,
    # so they agree to 2 ulp of a double.
    all_idx = np.concatenate([d[0] for d in drawn])
    all_pri = np.concatenate([d[1] for d in drawn])
    uniq, first, counts = np.unique(all_idx, return_index=True,
                                    return_counts=True)
    once = first[counts == 1]
    assert len(once) >= 8
    leaf = st[cap + all_idx[once]]
    want = np.array([float(p) ** ALPHA for p in all_pri[once]])
    np.testing.assert_allclose(leaf, want, rtol=2.0 ** -51, atol=0)
    assert np.array_equal(mt[cap + all_idx[once]], leaf)
    # never-drawn leaves are untouched
    rest = np.setdiff1d(np.arange(700), all_idx)
    assert np.array_equal(st[cap + rest], st0[cap + rest])
    assert (st[cap + 700:] == 0).all() and np.isinf(mt[cap + 700:]).all()
    assert eng.counters()["max_priority"] == float(run_max)
