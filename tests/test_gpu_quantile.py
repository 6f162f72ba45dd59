"""The quantile-regression critic head on the fused engine, all three train
paths: row formulas against a float64 oracle built from the engine's own
read-back, one and three steps against eager torch, the bitwise equalities the
categorical head has, checkpoints, and the untouched default.

Inputs reach every branch of the loss: rewards over [-3, 3] (|u| on both sides
of kappa = 1, both signs), a few done rows, and u == 0 planted exactly: the
critic's quantile 0 is the constant 0.5 (zero fc3 column, bias 0.5), the
target critic's quantile 0 the constant 0, so T_0 = r + gamma_n (1 - d) * 0 = r
exactly, and half of the rows carry r = 0.5.  Each shape's first step is
run once and shared (module cache); nothing mutates it.
"""

import copy
import functools
import math

import numpy as np
import pytest
import torch

import _engine_kit as kit
from _engine_kit import SLABS

pytestmark = pytest.mark.gpu

O, A = 5, 2
GAMMA_N = 0.99 ** 3
KAPPA = 1.0
TAU, LR = 0.01, 1e-4
PER_EPS = 1e-6
N = 1024
U2 = 2.0 ** -24
BUFFERS = ["sum_tree", "min_tree", "bidx", "pri", "bw", "br", "bd", "ba",
           "bs2", "p_t", "m_proj", "q", "dlog"]

SHAPES = {
    "persistent-8": dict(B=8, H=64, K=11),
    "persistent-50": dict(B=50, H=128, K=51),      # partial row group
    "persistent-64": dict(B=64, H=64, K=64),       # full wave
    "rowblock-260": dict(B=260, H=64, K=51),
    "wide-520": dict(B=520, H=64, K=51),           # edge tiles
    "wide-520-bf16": dict(B=520, H=64, K=51, gemm_precision="bf16"),
}
FP32_SHAPES = [k for k in SHAPES if not k.endswith("bf16")]


def _dist(K):
    return {"type": "quantile", "n_atoms": K, "kappa": KAPPA}


def _shape(name):
    s = SHAPES[name]
    return kit.Shape(s["B"], s["H"], O, A, s["K"], head="quantile",
                     precision=s.get("gemm_precision", "fp32"), kappa=KAPPA,
                     v_min=-1.0, v_max=1.0)


def _modules(name):
    a, at, c, _ = kit.modules(_shape(name), seed=SHAPES[name]["B"])
    with torch.no_grad():
        # quantiles spread over about [-2, 2] (the 3e-3 output init would
        # leave every u_ij of a row with the sign of r)
        c.fc3.weight.normal_(0.0, 2.0 / math.sqrt(SHAPES[name]["H"]))
        c.fc3.weight[0].zero_()
        c.fc3.bias[0] = 0.5
    ct = copy.deepcopy(c)
    with torch.no_grad():
        ct.fc3.bias[0] = 0.0
    return a, at, c, ct


def _transitions(seed=0):
    # its own generator: r and the mask of the reward atom are drawn BEFORE
    # s, which the kit's s, a, r, s2, d order cannot reproduce
    rng = np.random.default_rng(seed)
    r = rng.uniform(-3, 3, N).astype("f")
    r[rng.random(N) < 0.5] = 0.5
    return (rng.standard_normal((N, O)).astype("f"),
            rng.uniform(-1, 1, (N, A)).astype("f"), r,
            rng.standard_normal((N, O)).astype("f"),
            (rng.random(N) < 0.1).astype("f"))


def _engine(name, mods, tr, **kw):
    return kit.engine(_shape(name), mods, tr, capacity=N, gamma_n=GAMMA_N,
                      tau=TAU, lr=LR, per_eps=PER_EPS, **kw)


def _fresh(name, **kw):
    # the data seed is chosen so that even the B = 8 batch of the first step
    # (PER draw of seed 13 over 1024 equal leaves) holds a done row and rows
    # with r = 0.5; test_row_formulas asserts the counts
    mods = _modules(name)
    tr = _transitions(seed=SHAPES[name]["B"] + 2000)
    return _engine(name, mods, tr, **kw), mods, tr


READ = ["q", "p_t", "m_proj", "br", "bd", "bw", "dlog", "pri", "pd3", "a2",
        "bidx"]


@functools.lru_cache(maxsize=None)
def _first_step(name):
    """One step of a fresh engine of this shape: read-back, slabs, counters
    (shared by the tests below; treat as read-only)."""
    eng, mods, tr = _fresh(name, is_weighting=True)
    info = dict(eng.info())
    eng.step(1)
    out = {n: eng.read(n).numpy() for n in READ}
    slabs = {n: eng.store_slab(n).numpy() for n in SLABS}
    return out, slabs, eng.counters(), mods, tr, info


def _state(eng):
    return kit.snapshot(eng, BUFFERS)


_assert_same = kit.assert_bitwise


# ---------------------------------------------------------------------------
# 1. row formulas against a float64 oracle from the engine's own read-back
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(SHAPES))
def test_row_formulas_against_float64_oracle(name):
    """Measured on MI355X: see PARITY.md, "Quantile critic"."""
    o, _, cnt, _, _, info = _first_step(name)
    B, K = SHAPES[name]["B"], SHAPES[name]["K"]
    assert info["dist"] == "quantile" and info["kappa"] == KAPPA
    assert info["persistent"] == name.startswith("persistent")
    f8 = lambda x: np.asarray(x, np.float64)
    q, p_t, T = f8(o["q"]), f8(o["p_t"]), f8(o["m_proj"])
    r, d, w = f8(o["br"]), f8(o["bd"]), f8(o["bw"])
    g = float(np.float32(GAMMA_N))
    assert set(np.unique(d)) <= {0.0, 1.0} and d.sum() >= 1
    assert np.isfinite(q).all() and np.isfinite(p_t).all()

    # target samples from theta' (p_t)
    T_or = r[:, None] + g * (1.0 - d)[:, None] * p_t
    t_bound = 3 * U2 * (np.abs(r)[:, None] + g * np.abs(p_t))
    t_err = np.abs(T - T_or)
    print(f"{name}: T max err/bound {np.max(t_err / np.maximum(t_bound, 1e-300)):.3g}")

    # pairwise terms from the float values the engine used: T (m_proj) and
    # theta (q) as read back, so the sign of every u_ij is the engine's
    u = T[:, None, :] - q[:, :, None]                     # [B, i, j]
    small, large = np.abs(u) < KAPPA, np.abs(u) > KAPPA
    neg, zero = u < 0, u == 0
    counts = dict(small=int(small.sum()), large=int(large.sum()),
                  neg=int(neg.sum()), zero=int(zero.sum()))
    both = ((neg.any(axis=(1, 2))) & ((u > 0).any(axis=(1, 2)))).mean()
    print(f"{name}: branch counts {counts}, rows with both signs {both:.2f}")
    for k, v in counts.items():
        assert v > 0, (k, counts)
    assert both > 0.5

    tau = (2 * np.arange(K) + 1) / (2.0 * K)
    wgt = np.where(neg, 1.0 - tau[None, :, None], tau[None, :, None])
    cl = np.clip(u, -KAPPA, KAPPA)
    rowscale = w / (B * K)
    dlog_or = rowscale[:, None] * -(wgt * cl / KAPPA).sum(axis=2)
    d_bound = ((K + 8) * U2 * rowscale[:, None]
               * (wgt * np.abs(cl) / KAPPA).sum(axis=2))
    d_err = np.abs(f8(o["dlog"]) - dlog_or)
    print(f"{name}: dlog max err/bound "
          f"{np.max(d_err / np.maximum(d_bound, 1e-300)):.3g}")

    eps = float(np.float32(PER_EPS))
    pri_or = np.abs(T.mean(axis=1) - q.mean(axis=1)) + eps
    p_bound = 16 * U2 * (np.abs(T).sum(axis=1) + np.abs(q).sum(axis=1)) / K
    p_err = np.abs(f8(o["pri"]) - pri_or)
    print(f"{name}: pri max err/bound {np.max(p_err / p_bound):.3g}")

    assert (t_err <= t_bound).all()
    assert (d_err <= d_bound).all()
    assert (p_err <= p_bound).all()
    assert (o["pri"] >= np.float32(PER_EPS)).all()
    assert np.array_equal(
        o["pd3"], np.full((B, K), np.float32(-1.0) / np.float32(B * K)))

    # the loss scalars: (1/B) sum_b w_b l_b and -(1/B) sum_b mean_i theta_i
    # of the policy chain (pq is not q; only its finiteness is checked here)
    au = np.abs(u)
    hub = np.where(au <= KAPPA, 0.5 * u * u, KAPPA * (au - 0.5 * KAPPA))
    loss = (w * (wgt * hub / KAPPA).sum(axis=(1, 2)) / K).mean()
    assert cnt["loss_critic"] == pytest.approx(loss, rel=1e-4)
    assert np.isfinite(cnt["loss_actor"])


# ---------------------------------------------------------------------------
# 2. against the eager oracle
# ---------------------------------------------------------------------------

class Eager(kit.Eager):
    def __init__(self, mods):
        super().__init__(mods, LR, TAU,
                         head=kit.QuantileHead(GAMMA_N, KAPPA))

    def slabs(self):
        return dict(super().slabs(), **self.grads())


def _check_slabs(got, want, steps, tag):
    """The tolerances of test_gpu_multistep.py: parameters 2e-5 per step,
    gradients 1e-4 and 1e-3 of the slab's largest entry, moments also 1e-4
    of the slab's largest entry."""
    for n in SLABS:
        err = np.abs(got[n] - want[n]).max()
        print(f"{tag} {n}: max abs err {err:.3g} "
              f"(max |ref| {np.abs(want[n]).max():.3g})")
    for n in SLABS:
        scale = np.abs(want[n]).max()
        err = np.abs(got[n] - want[n]).max()
        if n.startswith("g_"):
            assert err <= 1e-4 and err <= 1e-3 * scale, n
        else:
            assert err <= 2e-5 * steps, n
        if n[:2] in ("m_", "v_"):
            assert err <= 1e-4 * scale, n


@pytest.mark.parametrize("name", FP32_SHAPES)
def test_one_step_matches_eager(name):
    o, slabs, _, mods, tr, _ = _first_step(name)
    eager = Eager(mods)
    eager.step(*[t[o["bidx"]] for t in tr], w=o["bw"])
    # test_gpu_shapes.py's tolerances for the same quantities
    np.testing.assert_allclose(o["a2"], eager.a2.numpy(), atol=5e-5)
    np.testing.assert_allclose(o["p_t"], eager.p_t.numpy(), atol=5e-5)
    np.testing.assert_allclose(o["m_proj"], eager.T.numpy(), atol=1e-4)
    np.testing.assert_allclose(o["q"], eager.q.detach().numpy(), atol=5e-5)
    _check_slabs(slabs, eager.slabs(), 1, name)


@pytest.mark.parametrize("name", ["persistent-8", "rowblock-260"])
def test_three_steps_match_eager(name):
    eng, mods, tr = _fresh(name)
    eager = Eager(mods)
    for _ in range(3):
        eng.step(1)
        idx = eng.read("bidx").numpy()
        eager.step(*[t[idx] for t in tr])
    got = {n: eng.store_slab(n).numpy() for n in SLABS}
    _check_slabs(got, eager.slabs(), 3, name + " x3")


# ---------------------------------------------------------------------------
# 3. bitwise equalities
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["persistent-8", "persistent-64"])
def test_multistep_launch_matches_single_steps(name):
    x, mods, tr = _fresh(name)
    y = _engine(name, mods, tr)
    assert x._persistent
    x.step(4)
    for _ in range(4):
        y.step(1)
    _assert_same(_state(x), _state(y), "step(4) vs 4 x step(1)")
    assert x.counters()["adam_t_critic"] == 4


def test_graph_replay_matches_uncaptured_rowblock():
    x, mods, tr = _fresh("rowblock-260")
    y = _engine("rowblock-260", mods, tr)
    assert not x._persistent
    x.step(4)
    y.train_steps(4, steps_per_graph=2)
    assert y._captured == 2
    _assert_same(_state(x), _state(y), "step(4) vs graph 2 x 2")


@pytest.mark.parametrize("name", ["rowblock-260", "wide-520"])
def test_split_step_matches_full_step(name):
    x, mods, tr = _fresh(name)
    y = _engine(name, mods, tr)
    x.step(1)
    for mask in (y.PH_CRITIC_GRADS, y.PH_CRITIC_APPLY, y.PH_ACTOR_GRADS,
                 y.PH_ACTOR_APPLY):
        y.step_part(mask)
    _assert_same(_state(x), _state(y), "step(1) vs four step_part")


def test_two_fresh_engines_agree():
    x, mods, tr = _fresh("persistent-50")
    y = _engine("persistent-50", mods, tr)
    x.step(3)
    y.step(3)
    _assert_same(_state(x), _state(y), "two fresh engines")


def test_grad_clip_with_quantile():
    x, mods, tr = _fresh("persistent-8", max_grad_norm=0.05)
    y = _engine("persistent-8", mods, tr, max_grad_norm=0.05)
    x.step(2)
    y.step(2)
    _assert_same(_state(x), _state(y), "clip-on quantile")
    for n in ("gn_part_actor", "gn_part_critic"):
        assert np.array_equal(x.read(n).numpy(), y.read(n).numpy()), n
    gs = x.grad_stats()
    for net in ("actor", "critic"):
        part = x.read("gn_part_" + net).numpy()
        assert gs["norm_" + net] == pytest.approx(math.sqrt(part.sum()),
                                                  rel=1e-12)
        assert 0.0 < gs["scale_" + net] <= 1.0
    assert gs["scale_critic"] < 1.0        # the threshold really clips


# ---------------------------------------------------------------------------
# 4. checkpoint
# ---------------------------------------------------------------------------

def _agent(dist, seed=0):
    return kit.agent(dist, memory_size=4096, hidden=64, seed=seed)


def _fill(agent, n=1000):
    kit.fill_agent(agent, n, reward=lambda rng: rng.uniform(-3, 3),
                   done=lambda rng: float(rng.random() < 0.1))


_flat_params = kit.flat_params


def test_checkpoint_resume_bitwise_and_kind_mismatch():
    a1 = _agent(_dist(51))
    _fill(a1)
    for _ in range(3):
        a1.train()
    st = a1.state_dict()
    assert st["engine"]["dist"] == "quantile"
    assert st["engine"]["kappa"] == KAPPA
    for _ in range(3):
        a1.train()
    ref = _flat_params(a1)

    a2 = _agent(_dist(51), seed=99)
    a2.load_state_dict(st)
    assert a2.engine.engine.info()["dist"] == "quantile"
    for _ in range(3):
        a2.train()
    np.testing.assert_array_equal(_flat_params(a2), ref)

    cat = _agent(kit.CATEGORICAL, seed=5)
    with pytest.raises(ValueError, match="critic head"):
        cat.load_state_dict(st)
    # and the other way round
    _fill(cat, n=200)
    cat.train()
    with pytest.raises(ValueError, match="critic head"):
        _agent(_dist(51), seed=6).load_state_dict(cat.state_dict())


# ---------------------------------------------------------------------------
# 5. the default is untouched; refusals
# ---------------------------------------------------------------------------

def test_default_dist_is_categorical_and_ignores_kappa():
    from d4pg_amd.models import actor, critic
    from d4pg_amd.ops import FusedEngine
    H, K, B = 64, 51, 64
    cdist = {"type": "categorical", "v_min": -30.0, "v_max": 5.0,
             "n_atoms": K}
    torch.manual_seed(1)
    a, c = actor(O, A, hidden=H), critic(O, A, cdist, hidden=H)
    mods = (a, copy.deepcopy(a), c, copy.deepcopy(c))
    tr = _transitions(seed=1)

    def make(**kw):
        eng = FusedEngine(obs_dim=O, act_dim=A, hidden=H, n_atoms=K, batch=B,
                          capacity=N, v_min=-30.0, v_max=5.0, gamma_n=GAMMA_N,
                          tau=TAU, lr_actor=LR, lr_critic=LR, seed=13, **kw)
        eng.load_from_modules(*mods)
        eng.ingest(*[torch.from_numpy(x) for x in tr])
        eng.step(4)
        return eng

    plain = make()
    info = plain.info()
    assert info["dist"] == "categorical" and info["kappa"] == 1.0
    ref = _state(plain)
    _assert_same(_state(make(dist="categorical")), ref, "explicit dist")
    _assert_same(_state(make(dist="categorical", kappa=0.25)), ref,
                 "categorical ignores kappa")
    # rows are probabilities: the softmax head is still there
    assert np.abs(plain.read("q").numpy().sum(axis=1) - 1).max() < 1e-4


def test_engine_refusals():
    from d4pg_amd.ops import FusedEngine

    def make(**kw):
        kw.setdefault("n_atoms", 11)
        return FusedEngine(obs_dim=O, act_dim=A, hidden=64, batch=8,
                           capacity=64, v_min=-1.0, v_max=1.0,
                           gamma_n=GAMMA_N, tau=TAU, lr_actor=LR,
                           lr_critic=LR, **kw)

    with pytest.raises(RuntimeError, match="dist"):
        make(dist="mixture_of_gaussian")
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(RuntimeError, match="kappa"):
            make(dist="quantile", kappa=bad)
    with pytest.raises(RuntimeError, match="n_atoms"):
        make(dist="quantile", n_atoms=65)
