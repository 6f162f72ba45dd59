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

import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

O, A, H, K = 5, 2, 128, 51
V_MIN, V_MAX = -300.0, 0.0
GAMMA_N = 0.99 ** 5
TAU, LR = 0.001, 1e-4
DIST = {"type": "categorical", "v_min": V_MIN, "v_max": V_MAX, "n_atoms": K}
N = 512
LAYERS = ["fc1", "fc2", "fc2_2", "fc3"]
SLABS = ["actor", "actor_target", "critic", "critic_target", "g_actor",
         "g_critic", "m_actor", "v_actor", "m_critic", "v_critic"]
BUFFERS = ["sum_tree", "min_tree", "bidx", "pri", "bw", "br", "bd", "ba",
           "bs2", "m_proj", "q"]
INT_COUNTERS = ["beta_t", "adam_t_actor", "adam_t_critic", "rng_epoch",
                "size", "pos"]


def _modules(seed=0):
    from d4pg_amd.models import actor, critic
    torch.manual_seed(seed)
    a = actor(O, A, hidden=H)
    c = critic(O, A, DIST, hidden=H)
    return a, copy.deepcopy(a), c, copy.deepcopy(c)


def _transitions(seed=0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((N, O)).astype("f"),
            rng.uniform(-1, 1, (N, A)).astype("f"),
            rng.uniform(-30, 0, N).astype("f"),
            rng.standard_normal((N, O)).astype("f"),
            (rng.random(N) < 0.05).astype("f"))


def _engine(B, mods, tr, seed=13):
    from d4pg_amd.ops import FusedEngine
    eng = FusedEngine(obs_dim=O, act_dim=A, hidden=H, n_atoms=K, batch=B,
                      capacity=N, v_min=V_MIN, v_max=V_MAX, gamma_n=GAMMA_N,
                      tau=TAU, lr_actor=LR, lr_critic=LR, seed=seed)
    eng.load_from_modules(*mods)
    eng.ingest(*[torch.from_numpy(x) for x in tr])
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


def _assert_bs_is_gathered(eng, what):
    """read('bs') resolves the parity buffer the last step used."""
    idx = eng.read("bidx").numpy()
    assert np.array_equal(eng.read("bs").numpy(), eng.replay_rows()[0][idx]), \
        f"{what}: bs is not the gathered batch"


# ---------------------------------------------------------------------------
# eager torch replica of one train step on a given batch
# ---------------------------------------------------------------------------

def _pack(module, get):
    """Flatten per-parameter tensors into the engine slab layout."""
    parts = []
    for n in LAYERS:
        lin = getattr(module, n)
        parts.append(get(lin.weight).t().contiguous().reshape(-1))
        parts.append(get(lin.bias).reshape(-1))
    return torch.cat(parts).detach().numpy()


class Eager:
    def __init__(self, mods):
        self.a, self.at, self.c, self.ct = [copy.deepcopy(m) for m in mods]
        self.opt_c = torch.optim.Adam(self.c.parameters(), lr=LR)
        self.opt_a = torch.optim.Adam(self.a.parameters(), lr=LR)

    def step(self, s, act, r, s2, d):
        """critic Adam, policy gradient through the UPDATED critic, actor
        Adam, both soft updates (test_post_step_params_parity's order)."""
        from d4pg_amd.algo.projection import categorical_projection
        s, act, r, s2, d = [torch.from_numpy(x) for x in (s, act, r, s2, d)]
        with torch.no_grad():
            m = categorical_projection(self.ct(s2, self.at(s2)), r, d, V_MIN,
                                       V_MAX, GAMMA_N)
        q = self.c(s, act)
        loss_c = -(m * torch.log(q + 1e-10)).sum(1).mean()
        self.c.zero_grad()
        loss_c.backward()
        # (the policy loss below also backpropagates into the critic)
        self.g_critic = _pack(self.c, lambda p: p.grad.clone())
        self.opt_c.step()
        z = torch.linspace(V_MIN, V_MAX, K).reshape(-1, 1)
        pl = -(self.c(s, self.a(s)).matmul(z)).mean()
        self.a.zero_grad()
        pl.backward()
        self.opt_a.step()
        with torch.no_grad():
            for tp, sp in zip(self.at.parameters(), self.a.parameters()):
                tp.lerp_(sp, TAU)
            for tp, sp in zip(self.ct.parameters(), self.c.parameters()):
                tp.lerp_(sp, TAU)

    def grads(self):
        """Gradients of the LAST step, in the engine's slab layout."""
        return {"g_actor": _pack(self.a, lambda p: p.grad),
                "g_critic": self.g_critic}

    def slabs(self):
        out = {"actor": _pack(self.a, lambda p: p),
               "actor_target": _pack(self.at, lambda p: p),
               "critic": _pack(self.c, lambda p: p),
               "critic_target": _pack(self.ct, lambda p: p)}
        for tag, net, opt in (("actor", self.a, self.opt_a),
                              ("critic", self.c, self.opt_c)):
            out["m_" + tag] = _pack(net, lambda p: opt.state[p]["exp_avg"])
            out["v_" + tag] = _pack(net, lambda p: opt.state[p]["exp_avg_sq"])
        return out


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
