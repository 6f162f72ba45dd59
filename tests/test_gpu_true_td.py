"""True-TD priorities on the fused engine (FusedEngine(true_td_priorities=
True)): the row priority is |E_m[z] - E_q[z]| + per_eps, the eager formula of
algo/d4pg.py, in place of the reference's <m, q> proxy.

The bound on the priority is derived, not tuned.  Each expectation is a
64-lane butterfly sum (6 levels) of products p_k z_k with sum(p) = 1 and
|z| <= Z = max(|v_min|, |v_max|): at most 7 roundings of magnitude <= Z
2^-24 each (one per product, one per level), twice; the float32 atom
v_min + k delta adds under 2 ulp of Z per expectation, and the final
subtraction and + eps one each: 20 * 2^-24 * Z in all (3.6e-4 on [-300, 0]).
"""

import copy

import numpy as np
import pytest

import _engine_kit as kit

pytestmark = pytest.mark.gpu

# the shape, seed and injected replay of test_gpu_per_exact.py
O, A, H, K = 5, 2, 128, 51
V_MIN, V_MAX = -300.0, 0.0
GAMMA_N = 0.99 ** 5
ALPHA = float(np.float32(0.6))          # the engine holds per_alpha as float
SEED = 21
PER_EPS = 1e-6
ATOL = 20 * 2.0 ** -24 * max(abs(V_MIN), abs(V_MAX))
Z = np.linspace(V_MIN, V_MAX, K)            # float64 atoms
_inject = kit.inject_replay


def _shape(B=0):
    return kit.Shape(B, H, O, A, K)


DIST = _shape().dist


def _engine(B, capacity, true_td=True):
    return kit.engine(_shape(B), capacity=capacity, seed=SEED,
                      per_eps=PER_EPS, true_td_priorities=true_td)


def _modules(seed=0):
    return kit.modules(_shape(), seed)


def _replay(size, seed=0):
    return kit.per_replay(_shape(), size, seed)


def _td64(m, q):
    m, q = m.astype(np.float64), q.astype(np.float64)
    return np.abs((m * Z).sum(1) - (q * Z).sum(1)) + PER_EPS


class _Recorder:
    """Stands in for the eager agent's replay: keeps the priorities the
    train step writes back."""
    def update_priorities(self, idxes, priorities):
        self.priorities = np.asarray(priorities)


def _eager_priorities(mods, batch, true_td):
    from d4pg_amd.algo.d4pg import DDPG
    agent = DDPG(O, A, memory_size=16, batch_size=len(batch["br"]),
                 critic_dist_info=DIST, n_steps=5, gamma=0.99,
                 prioritized_replay=True, hidden=H,
                 true_td_priorities=true_td)
    assert agent.n_step_gamma == GAMMA_N
    for net, src in zip((agent.actor, agent.actor_target, agent.critic,
                         agent.critic_target), mods):
        net.load_state_dict(copy.deepcopy(src.state_dict()))
    agent.replayBuffer = rec = _Recorder()
    B = len(batch["br"])
    agent._train_step_eager((batch["bs"], batch["ba"], batch["br"],
                             batch["bs2"], batch["bd"], None, np.arange(B)))
    return rec.priorities


# persistent megakernel / row-block / per-layer MFMA path
@pytest.mark.parametrize("B", [64, 300, 640])
def test_priority_formula_and_writeback(B):
    """Measured on MI355X (PARITY.md): max |pri - float64| 3.2e-5, 2.7e-5,
    2.9e-5 at B = 64, 300, 640; against the eager agent 4.6e-5."""
    mods = _modules(seed=B)
    rp = _replay(700, seed=B)
    eng = _engine(B, 1024)
    assert eng.info()["true_td"] is True and eng.info()["prioritized"] is True
    eng.load_from_modules(*mods)
    st0, _, cap = _inject(eng, rp)
    eng.step(1)
    o = {n: eng.read(n).numpy() for n in
         ["bs", "ba", "br", "bs2", "bd", "bidx", "q", "m_proj", "pri"]}
    want = _td64(o["m_proj"], o["q"])
    err = np.abs(o["pri"] - want).max()
    print(f"B={B}: max |pri - float64| = {err:.3g} (bound {ATOL:.3g}, "
          f"pri in [{want.min():.3g}, {want.max():.3g}])")
    # the test cannot pass on the proxy <m, q> + eps (nor without the abs:
    # both signs of E_m - E_q occur)
    proxy = (o["m_proj"].astype(np.float64) * o["q"]).sum(1) + PER_EPS
    assert (np.abs(want - proxy) > ATOL).mean() >= 0.25
    signed = ((o["m_proj"].astype(np.float64) * Z).sum(1)
              - (o["q"].astype(np.float64) * Z).sum(1))
    assert (signed > ATOL).sum() >= 8 and (signed < -ATOL).sum() >= 8
    np.testing.assert_allclose(o["pri"], want, rtol=0, atol=ATOL)

    # 9. the eager agent with true_td_priorities=True on the same batch
    eager = _eager_priorities(mods, o, True)
    err_e = np.abs(o["pri"] - eager).max()
    print(f"B={B}: max |pri - eager| = {err_e:.3g}")
    np.testing.assert_allclose(o["pri"], eager, rtol=0, atol=ATOL)

    # write-back: leaves drawn once carry pri^alpha (device and host pow each
    # within 1 ulp: 2 ulp of a double apart), parents are bitwise the sums
    st = eng.read("sum_tree").numpy()
    mt = eng.read("min_tree").numpy()
    n = np.arange(1, cap)
    assert np.array_equal(st[n], st[2 * n] + st[2 * n + 1])
    assert np.array_equal(mt[n], np.minimum(mt[2 * n], mt[2 * n + 1]))
    uniq, first, counts = np.unique(o["bidx"], return_index=True,
                                    return_counts=True)
    once = first[counts == 1]
    assert len(once) >= 8
    leaf = st[cap + o["bidx"][once]]
    wleaf = np.array([float(p) ** ALPHA for p in o["pri"][once]])
    np.testing.assert_allclose(leaf, wleaf, rtol=2.0 ** -51, atol=0)
    assert np.array_equal(mt[cap + o["bidx"][once]], leaf)
    rest = np.setdiff1d(np.arange(700), o["bidx"])
    assert np.array_equal(st[cap + rest], st0[cap + rest])
    # true TD errors exceed 1: the running maximum follows them
    assert eng.counters()["max_priority"] == float(
        max(np.float32(1.0), o["pri"].max()))


@pytest.mark.parametrize("B", [64, 300, 640])
def test_flag_changes_only_the_priority(B):
    """Same seed, same injected tree: with and without the flag the step's
    gradients and parameters are bitwise equal; only pri (and what is
    written back from it) differs."""
    mods = _modules(seed=B)
    rp = _replay(700, seed=B)
    out = {}
    for flag in (True, False):
        eng = _engine(B, 1024, true_td=flag)
        eng.load_from_modules(*mods)
        _inject(eng, rp)
        eng.step(1)
        o = {n: eng.read(n).numpy() for n in
             ["bidx", "bw", "q", "m_proj", "dlog", "pri"]}
        for n in ("g_critic", "g_actor", "critic", "actor"):
            o[n] = eng.store_slab(n).numpy()
        out[flag] = o
    t, p = out[True], out[False]
    for n in t:
        if n != "pri":
            assert np.array_equal(t[n], p[n]), n
    proxy = (p["m_proj"].astype(np.float64) * p["q"]).sum(1) + PER_EPS
    np.testing.assert_allclose(p["pri"], proxy, rtol=1e-5)
    assert (np.abs(t["pri"] - p["pri"]) > ATOL).mean() >= 0.25
