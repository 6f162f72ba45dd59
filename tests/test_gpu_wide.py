"""GPU parity for the wide-batch (MFMA) engine paths: B > 512 routes the
layer GEMMs through the matrix-core kernels (k_mfma_fwd/dx/dw, split-K,
per-level PER repair) — replicate one full step in eager fp32 torch on the
identical sampled batch and compare every stage."""

import copy

import numpy as np
import pytest
import torch

import _engine_kit as kit

pytestmark = pytest.mark.gpu

O, A, H, K = 17, 6, 128, 51
B = 1024
GAMMA_N = 0.99 ** 5
TAU = 0.001
LR = 1e-4


@pytest.fixture(scope="module")
def wstepped():
    shape = kit.Shape(B, H, O, A, K)
    a, at, c, ct = mods = kit.modules(shape, seed=5)
    eng = kit.engine(shape, mods, kit.transitions(shape, 4096, seed=7),
                     capacity=8192, seed=11)
    eng.step(1)
    out = {name: eng.read(name) for name in
           ["bs", "ba", "br", "bs2", "bd", "q", "p_t", "a2", "m_proj",
            "dlog", "pri", "sum_tree", "bidx"]}
    out["counters"] = eng.counters()
    out["slab_actor"] = eng.store_slab("actor")
    out["slab_critic"] = eng.store_slab("critic")
    out["g_actor"] = eng.store_slab("g_actor")
    out["g_critic"] = eng.store_slab("g_critic")
    out["tree_cap"] = eng.info()["tree_cap"]
    return {"out": out, "modules": (a, at, c, ct)}


def test_wide_forward_projection_parity(wstepped):
    from d4pg_amd.algo.projection import categorical_projection
    o = wstepped["out"]
    a, at, c, ct = wstepped["modules"]
    s = torch.from_numpy(o["bs"].numpy())
    act = torch.from_numpy(o["ba"].numpy())
    r = torch.from_numpy(o["br"].numpy())
    s2 = torch.from_numpy(o["bs2"].numpy())
    d = torch.from_numpy(o["bd"].numpy())
    with torch.no_grad():
        a2 = at(s2)
        p_t = ct(s2, a2)
        m = categorical_projection(p_t, r, d, -300.0, 0.0, GAMMA_N)
        q = c(s, act)
    np.testing.assert_allclose(o["a2"].numpy(), a2.numpy(), atol=5e-5)
    np.testing.assert_allclose(o["p_t"].numpy(), p_t.numpy(), atol=5e-5)
    np.testing.assert_allclose(o["m_proj"].numpy(), m.numpy(), atol=1e-4)
    np.testing.assert_allclose(o["q"].numpy(), q.numpy(), atol=5e-5)


def test_wide_post_step_parity(wstepped):
    from d4pg_amd.algo.projection import categorical_projection
    from d4pg_amd.ops import pack_net
    o = wstepped["out"]
    a, at, c, ct = [copy.deepcopy(m) for m in wstepped["modules"]]
    s = torch.from_numpy(o["bs"].numpy())
    act = torch.from_numpy(o["ba"].numpy())
    r = torch.from_numpy(o["br"].numpy())
    s2 = torch.from_numpy(o["bs2"].numpy())
    d = torch.from_numpy(o["bd"].numpy())

    opt_c = torch.optim.Adam(c.parameters(), lr=LR)
    opt_a = torch.optim.Adam(a.parameters(), lr=LR)
    with torch.no_grad():
        m = categorical_projection(ct(s2, at(s2)), r, d, -300.0, 0.0,
                                   GAMMA_N)
    q = c(s, act)
    loss_c = -(m * torch.log(q + 1e-10)).sum(1).mean()
    c.zero_grad()
    loss_c.backward()
    gc = torch.cat([torch.cat([getattr(c, n).weight.grad.t().reshape(-1),
                               getattr(c, n).bias.grad])
                    for n in ["fc1", "fc2", "fc2_2", "fc3"]])
    np.testing.assert_allclose(o["g_critic"].numpy(), gc.numpy(), atol=1e-4)
    opt_c.step()

    z = torch.linspace(-300.0, 0.0, K).reshape(-1, 1)
    pl = -(c(s, a(s)).matmul(z)).mean()
    a.zero_grad()
    pl.backward()
    ga = torch.cat([torch.cat([getattr(a, n).weight.grad.t().reshape(-1),
                               getattr(a, n).bias.grad])
                    for n in ["fc1", "fc2", "fc2_2", "fc3"]])
    np.testing.assert_allclose(o["g_actor"].numpy(), ga.numpy(), atol=1e-4)
    opt_a.step()

    np.testing.assert_allclose(o["slab_critic"].numpy(),
                               pack_net(c).numpy(), atol=5e-5)
    np.testing.assert_allclose(o["slab_actor"].numpy(),
                               pack_net(a).numpy(), atol=5e-5)


def test_wide_tree_writeback(wstepped):
    o = wstepped["out"]
    cap = o["tree_cap"]
    tree = o["sum_tree"].numpy()
    idx = o["bidx"].numpy()
    pri = o["pri"].numpy()
    # last write wins on duplicate indices; all sampled leaves must carry
    # SOME sampled priority^alpha and the root must equal the leaf sum
    leaves = tree[cap:cap + 4096]
    assert tree[1] == pytest.approx(leaves.sum(), rel=1e-9)
    uniq, counts = np.unique(idx, return_counts=True)
    single = uniq[counts == 1]
    lut = {i: p for i, p in zip(idx, pri)}
    for i in single[:64]:
        assert leaves[i] == pytest.approx(lut[i] ** 0.6, rel=1e-5)
    assert o["counters"]["adam_t_actor"] == 1


# ---------------------------------------------------------------------------
# the f32 MFMA GEMMs one by one (the harness of tests/_wide_gemm.py, which
# test_gpu_wide_bf16.py runs with bf16 operands): expected = a @ b (+ bias) in
# float64 from the engine's own fp32 inputs of that GEMM, bound
# (K + ksplit + 2) * 2^-23 * (|a| @ |b| + |bias|) — any order of fp32
# accumulation over K terms plus the split-K sum stays inside it.
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module", params=["a", "b", "c"])
def phased_fp32(request):
    from _wide_gemm import run_phased
    return run_phased(request.param, "fp32")


def test_fp32_critic_phase_gemm_by_gemm(phased_fp32):
    from _wide_gemm import check_critic_phase
    check_critic_phase(phased_fp32)


def test_fp32_actor_phase_gemm_by_gemm(phased_fp32):
    from _wide_gemm import check_actor_phase
    check_actor_phase(phased_fp32)
