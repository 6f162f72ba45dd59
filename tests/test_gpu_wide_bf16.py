"""The wide train step with gemm_precision="bf16" (ops/hip/engine_mfma_bf16.hip):
every GEMM reads both operands rounded to bf16 (round-to-nearest-even) and
accumulates in fp32; everything else is the fp32 step.

The GEMMs are checked one by one, teacher-forced: the expected value of each
is built from the engine's OWN fp32 input buffers of that GEMM, so a rounding
flip upstream cannot leak into the comparison,

    bf(x) = x.to(bfloat16).to(float64)
    expected = bf(a) @ bf(b) (+ fp32 bias)            in float64

Products of two bf16 values are exact in fp32, so the only error left is the
fp32 accumulation, bounded for ANY summation order by

    (K + ksplit + 2) * 2^-23 * (|bf(a)| @ |bf(b)| + |bias|)

elementwise (K the summed dimension, ksplit the split-K factor of that
launch; unit roundoff 2^-23 rather than 2^-24 also covers adds inside the
MFMA that do not round to nearest).  ReLU and the 0/1 ReLU mask do not grow
the bound; outputs behind tanh or softmax use the 5e-5 atol of
tests/test_gpu_wide.py.
"""

import numpy as np
import pytest
import torch

import _engine_kit as kit
from _wide_gemm import (CONFIGS, LR, Net, _engine, _gemm, _ks_dw,
                        _modules, _rows, check_actor_phase,
                        check_critic_phase, run_phased)

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------
# 1. teacher-forced, GEMM by GEMM (the harness is tests/_wide_gemm.py)
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module", params=sorted(CONFIGS))
def phased(request):
    return run_phased(request.param, "bf16")


def test_critic_phase_gemm_by_gemm(phased):
    check_critic_phase(phased)


def test_actor_phase_gemm_by_gemm(phased):
    check_actor_phase(phased)


# ---------------------------------------------------------------------------
# 2. the bf16 path is really taken
# ---------------------------------------------------------------------------

def test_fp32_engine_is_outside_the_bf16_bound():
    """The oracle of each named GEMM is built from the inputs of the engine it
    is compared with, so only that GEMM's own operand rounding is on trial:
    the bf16 engine lies inside the bound, a same-seed fp32 engine outside."""
    c = CONFIGS["a"]
    B = c["B"]
    res = {}
    for prec in ("bf16", "fp32"):
        eng = _engine(c, prec)
        assert eng.info()["gemm_precision"] == prec
        info = eng.info()
        cr = Net(eng.store_slab("critic"), info["critic_layers"])
        eng.step_part(eng.PH_CRITIC_GRADS)
        res[prec] = ({n: eng.read(n) for n in ["c_h1", "ba", "c_h2", "d2",
                                               "bidx"]},
                     Net(eng.store_slab("g_critic"), info["critic_layers"]),
                     cr)
    assert torch.equal(res["bf16"][0]["bidx"], res["fp32"][0]["bidx"])
    H = c["H"]
    outside = {}
    for prec, (h, g, cr) in res.items():
        x = torch.cat([h["c_h1"], h["ba"]], 1)
        exp, bound = _gemm(x, cr.w[1], x.shape[1], 1, cr.b[1])
        err = (h["c_h2"].double() - exp.clamp_min(0)).abs()
        outside[prec, "c_h2"] = bool((err > bound).any())
        exp, bound = _gemm(h["c_h1"].t(), h["d2"], B, _ks_dw(B, H, H))
        err = (g.w[1][:H].double() - exp).abs()
        outside[prec, "g_critic L2"] = bool((err > bound).any())
    for what in ("c_h2", "g_critic L2"):
        assert not outside["bf16", what], f"bf16 {what} is outside its bound"
        assert outside["fp32", what], f"fp32 {what} is inside the bf16 bound"


# ---------------------------------------------------------------------------
# 3. rounding mode, exact
# ---------------------------------------------------------------------------

def test_operands_round_to_nearest_even():
    c = CONFIGS["a"]
    O = c["O"]
    a, at, cr, ct = _modules(c)
    with torch.no_grad():
        cr.fc1.weight.zero_()
        cr.fc1.bias.zero_()
        cr.fc1.weight[:O, :O] = torch.eye(O)
    # bf16 keeps 8 significand bits: 1 + 2^-8 is a tie that rounds DOWN to
    # the even 1.0, 1 + 3 * 2^-8 a tie that rounds UP to the even 1 + 2^-6,
    # 1 + 2^-8 + 2^-20 lies just above the tie, and 0x0001C000 is an fp32
    # denormal that rounds up to the bf16 denormal 0x0002
    den = float(np.array([0x0001C000], np.uint32).view(np.float32)[0])
    vals = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8),
                     -(1 + 3 * 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -20, den],
                    np.float32)
    rng = np.random.default_rng(3)
    s, act, r, s2, d = _rows(c)
    s = vals[rng.integers(0, len(vals), s.shape)]
    eng = _engine(c, mods=(a, at, cr, ct), rows=(s, act, r, s2, d))
    eng.step_part(eng.PH_CRITIC_GRADS)
    bs = eng.read("bs")
    assert set(np.unique(bs.numpy()).tolist()) == set(vals.tolist())
    want = bs.to(torch.bfloat16).to(torch.float32).clamp_min(0)
    got = eng.read("c_h1")[:, :O].contiguous()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


# ---------------------------------------------------------------------------
# 4. determinism
# ---------------------------------------------------------------------------

def _slabs(eng):
    """The ten slabs as int32 words: -0.0 and NaN payloads count too."""
    st, _ = kit.snapshot(eng, [], counters=[])
    return {k: v.view(np.int32) for k, v in st.items()}


def _assert_slabs_equal(x, y, what):
    assert x.keys() == y.keys()
    for k in x:
        assert np.array_equal(x[k], y[k]), f"{what}: {k} differs"


def test_two_runs_are_bitwise_equal():
    c = CONFIGS["b"]
    out = []
    for _ in range(2):
        eng = _engine(c)
        eng.step(3)
        out.append(_slabs(eng))
    _assert_slabs_equal(out[0], out[1], "two engines, same seed, 3 steps")


def test_graph_replay_equals_uncaptured_steps():
    c = CONFIGS["b"]
    eng = _engine(c)
    eng.train_steps(4, steps_per_graph=2)
    ref = _engine(c)
    for _ in range(4):
        ref.step(1)
    _assert_slabs_equal(_slabs(eng), _slabs(ref), "graph replay vs step(1) x4")
    ce, cf = eng.counters(), ref.counters()
    for k in ("beta_t", "adam_t_actor", "adam_t_critic", "rng_epoch"):
        assert ce[k] == cf[k] == 4


# ---------------------------------------------------------------------------
# 5. the optimizer is the fp32 one
# ---------------------------------------------------------------------------

def test_adam_is_fp32_on_the_engines_gradients():
    c = CONFIGS["a"]
    eng = _engine(c)
    p0 = {n: eng.store_slab(n) for n in ("actor", "critic")}
    eng.step(1)
    for n in ("actor", "critic"):
        p = p0[n].clone().requires_grad_(True)
        p.grad = eng.store_slab("g_" + n)
        torch.optim.Adam([p], lr=LR).step()
        np.testing.assert_allclose(eng.store_slab(n).numpy(),
                                   p.detach().numpy(), atol=5e-5)


# ---------------------------------------------------------------------------
# 6. refusals and plumbing
# ---------------------------------------------------------------------------

def test_refuses_batch_512():
    c = CONFIGS["a"]
    with pytest.raises(RuntimeError, match="gemm_precision"):
        _engine(c, batch=512)


def test_unknown_precision_refused():
    with pytest.raises(ValueError, match="gemm_precision"):
        _engine(CONFIGS["a"], precision="fp16")


def test_eager_backend_refuses():
    from d4pg_amd.algo.d4pg import DDPG
    with pytest.raises(ValueError, match="gemm_precision"):
        DDPG(3, 1, backend="eager", gemm_precision="bf16")


def test_agent_builds_a_bf16_engine():
    from d4pg_amd.algo.d4pg import DDPG
    agent = DDPG(3, 1, memory_size=4096, batch_size=1024, device="cuda",
                 backend="hip", hidden=128, gemm_precision="bf16", seed=0)
    bridge = agent.ensure_engine()
    assert bridge.engine.info()["gemm_precision"] == "bf16"
    assert bridge.engine.gemm_precision == "bf16"
