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

import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GAMMA_N = 0.99 ** 5
TAU, LR = 0.001, 1e-4
V_MIN, V_MAX = -300.0, 0.0
N_ROWS = 4096
U = 2.0 ** -23
SLABS = ["actor", "actor_target", "critic", "critic_target", "g_actor",
         "g_critic", "m_actor", "v_actor", "m_critic", "v_critic"]

# a: aligned interior tiles, odd fan-in 17, concat 134, head 51 with split-K
# b: N edge tile 128+72, K tail of 8, B % 64 = 10, dW K = 650 (empty tail
#    split-K segments)
# c: H % 8 != 0, a single M edge tile
CONFIGS = {
    "a": dict(O=17, A=6, H=128, K=51, B=1024),
    "b": dict(O=11, A=3, H=200, K=21, B=650),
    "c": dict(O=3, A=1, H=100, K=51, B=520),
}

CRITIC_BUFS = ["bs", "ba", "bs2", "at_h1", "at_h2", "at_h3", "a2", "ct_h1",
               "ct_h2", "ct_h3", "p_t", "c_h1", "c_h2", "c_h3", "q", "dlog",
               "d1", "d2", "d3"]
ACTOR_BUFS = ["bs", "pa_h1", "pa_h2", "pa_h3", "a_out", "pc_h1", "pc_h2",
              "pc_h3", "pq", "pd3", "pd2", "pdh1", "pda", "adz", "az1", "az2",
              "az3"]


def _dist(c):
    return {"type": "categorical", "v_min": V_MIN, "v_max": V_MAX,
            "n_atoms": c["K"]}


def _modules(c, seed=5):
    from d4pg_amd.models import actor, critic
    torch.manual_seed(seed)
    a = actor(c["O"], c["A"], hidden=c["H"])
    cr = critic(c["O"], c["A"], _dist(c), hidden=c["H"])
    return a, copy.deepcopy(a), cr, copy.deepcopy(cr)


def _rows(c, seed=7):
    rng = np.random.default_rng(seed)
    n = N_ROWS
    return (rng.standard_normal((n, c["O"])).astype("f"),
            rng.uniform(-1, 1, (n, c["A"])).astype("f"),
            rng.uniform(-30, 0, n).astype("f"),
            rng.standard_normal((n, c["O"])).astype("f"),
            (rng.random(n) < 0.05).astype("f"))


def _engine(c, precision="bf16", mods=None, rows=None, seed=11, batch=None):
    from d4pg_amd.ops import FusedEngine
    eng = FusedEngine(obs_dim=c["O"], act_dim=c["A"], hidden=c["H"],
                      n_atoms=c["K"], batch=batch or c["B"], capacity=8192,
                      v_min=V_MIN, v_max=V_MAX, gamma_n=GAMMA_N, tau=TAU,
                      lr_actor=LR, lr_critic=LR, seed=seed,
                      gemm_precision=precision)
    eng.load_from_modules(*(mods or _modules(c)))
    eng.ingest(*[torch.from_numpy(x) for x in (rows or _rows(c))])
    return eng


# ---------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------

def bf(x):
    return x.to(torch.bfloat16).to(torch.float64)


def _gemm(a, b, k, ksplit, bias=None):
    """(expected, bound) of bf(a) @ bf(b) + bias, float64."""
    a, b = bf(a), bf(b)
    exp = a @ b
    mag = a.abs() @ b.abs()
    if bias is not None:
        exp = exp + bias.to(torch.float64)
        mag = mag + bias.to(torch.float64).abs()
    return exp, (k + ksplit + 2) * U * mag


def _close(got, exp, bound, what):
    err = (got.to(torch.float64) - exp).abs()
    worst = float((err - bound).max())
    print(f"{what}: max err {float(err.max()):.3e}, "
          f"max bound {float(bound.max()):.3e}")
    assert worst <= 0.0, f"{what}: error exceeds the bound by {worst:.3e}"


def _ceil(a, b):
    return (a + b - 1) // b


def _ks_head(B, in_total):
    """split-K factor of a narrow (out <= 64) forward head."""
    ntm, ks = _ceil(B, 64), 1
    while ntm * ks < 512 and ks * 64 <= in_total:
        ks *= 2
    return ks


def _ks_dw(B, in_n, out):
    """split-K factor of one dW GEMM."""
    nt, ks = _ceil(in_n, 64) * _ceil(out, 128), 1
    while nt * ks < 256 and ks * 64 <= B:
        ks *= 2
    return ks


class Net:
    """One net's slab cut into per-layer [in][out] weights and biases."""

    def __init__(self, slab, layers):
        self.layers = layers
        self.w, self.b = [], []
        for l in layers:
            n_in = l["in1"] + l["in2"]
            self.w.append(slab[l["w_off"]:l["w_off"] + n_in * l["out"]]
                          .reshape(n_in, l["out"]))
            self.b.append(slab[l["b_off"]:l["b_off"] + l["out"]])


def _check_fwd(buf, net, i, x, got, act, B, what):
    l = net.layers[i]
    n_in = l["in1"] + l["in2"]
    ks = _ks_head(B, n_in) if l["out"] <= 64 else 1
    exp, bound = _gemm(x, net.w[i], n_in, ks, net.b[i])
    if act == "relu":
        exp = exp.clamp_min(0)
    elif act == "tanh":
        exp, bound = exp.tanh(), torch.full_like(exp, 5e-5)
    elif act == "softmax":
        exp, bound = exp.softmax(1), torch.full_like(exp, 5e-5)
    _close(buf[got], exp, bound, what)


def _check_dx(net, i, dz, mask_h, got, what):
    """dx1 = (dz @ W[:in1]^T) * relu'(mask_h)."""
    l = net.layers[i]
    exp, bound = _gemm(dz, net.w[i][:l["in1"]].t(), l["out"], 1)
    if mask_h is not None:
        m = (mask_h > 0).to(torch.float64)
        exp, bound = exp * m, bound * m
    _close(got, exp, bound, what)


def _check_dw(net, g, i, dz, x1, x2, B, what):
    """The layer's block of the gradient slab: dWt (per input block, as the
    engine runs it) and db."""
    l = net.layers[i]
    gnet = Net(g, net.layers)
    lo = 0
    for x in (x1, x2):
        if x is None:
            continue
        n = x.shape[1]
        ks = _ks_dw(B, n, l["out"])
        exp, bound = _gemm(x.t(), dz, B, ks)
        _close(gnet.w[i][lo:lo + n], exp, bound, f"{what} dW[{lo}:{lo + n}]")
        lo += n
    ks = _ks_dw(B, l["in1"], l["out"])
    exp, bound = _gemm(torch.ones(1, B), dz, B, ks)
    _close(gnet.b[i], exp[0], bound[0], f"{what} db")


# ---------------------------------------------------------------------------
# 1. teacher-forced, GEMM by GEMM
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module", params=sorted(CONFIGS))
def phased(request):
    """One bf16 engine per config, stepped phase by phase; every buffer and
    slab read after the phase that wrote it."""
    c = CONFIGS[request.param]
    eng = _engine(c)
    info = eng.info()
    assert info["gemm_precision"] == "bf16"
    st = {"cfg": c, "name": request.param, "info": info}
    st["slabs0"] = {n: eng.store_slab(n) for n in SLABS}
    eng.step_part(eng.PH_CRITIC_GRADS)
    st["critic"] = {n: eng.read(n) for n in CRITIC_BUFS}
    st["g_critic"] = eng.store_slab("g_critic")
    eng.step_part(eng.PH_CRITIC_APPLY)
    st["p_critic1"] = eng.store_slab("critic")
    eng.step_part(eng.PH_ACTOR_GRADS)
    st["actor"] = {n: eng.read(n) for n in ACTOR_BUFS}
    st["g_actor"] = eng.store_slab("g_actor")
    return st


def test_critic_phase_gemm_by_gemm(phased):
    c, buf, info = phased["cfg"], phased["critic"], phased["info"]
    B = c["B"]
    s0 = phased["slabs0"]
    at = Net(s0["actor_target"], info["actor_layers"])
    ct = Net(s0["critic_target"], info["critic_layers"])
    cr = Net(s0["critic"], info["critic_layers"])
    cat = lambda a, b: torch.cat([buf[a], buf[b]], 1)
    fwd = lambda *a: _check_fwd(buf, *a)
    # target actor
    fwd(at, 0, buf["bs2"], "at_h1", "relu", B, "at.L1")
    fwd(at, 1, buf["at_h1"], "at_h2", None, B, "at.L2")
    fwd(at, 2, buf["at_h2"], "at_h3", "relu", B, "at.L3")
    fwd(at, 3, buf["at_h3"], "a2", "tanh", B, "at.L4")
    # target critic
    fwd(ct, 0, buf["bs2"], "ct_h1", "relu", B, "ct.L1")
    fwd(ct, 1, cat("ct_h1", "a2"), "ct_h2", "relu", B, "ct.L2")
    fwd(ct, 2, buf["ct_h2"], "ct_h3", "relu", B, "ct.L3")
    fwd(ct, 3, buf["ct_h3"], "p_t", "softmax", B, "ct.L4")
    # critic
    fwd(cr, 0, buf["bs"], "c_h1", "relu", B, "c.L1")
    fwd(cr, 1, cat("c_h1", "ba"), "c_h2", "relu", B, "c.L2")
    fwd(cr, 2, buf["c_h2"], "c_h3", "relu", B, "c.L3")
    fwd(cr, 3, buf["c_h3"], "q", "softmax", B, "c.L4")
    # critic backward
    _check_dx(cr, 3, buf["dlog"], buf["c_h3"], buf["d3"], "c.L4 dX")
    _check_dx(cr, 2, buf["d3"], buf["c_h2"], buf["d2"], "c.L3 dX")
    _check_dx(cr, 1, buf["d2"], buf["c_h1"], buf["d1"], "c.L2 dX")
    g = phased["g_critic"]
    _check_dw(cr, g, 3, buf["dlog"], buf["c_h3"], None, B, "c.L4")
    _check_dw(cr, g, 2, buf["d3"], buf["c_h2"], None, B, "c.L3")
    _check_dw(cr, g, 1, buf["d2"], buf["c_h1"], buf["ba"], B, "c.L2")
    _check_dw(cr, g, 0, buf["d1"], buf["bs"], None, B, "c.L1")


def test_actor_phase_gemm_by_gemm(phased):
    c, buf, info = phased["cfg"], phased["actor"], phased["info"]
    B = c["B"]
    ac = Net(phased["slabs0"]["actor"], info["actor_layers"])
    cr = Net(phased["p_critic1"], info["critic_layers"])  # after its Adam
    fwd = lambda *a: _check_fwd(buf, *a)
    fwd(ac, 0, buf["bs"], "pa_h1", "relu", B, "a.L1")
    fwd(ac, 1, buf["pa_h1"], "pa_h2", None, B, "a.L2")
    fwd(ac, 2, buf["pa_h2"], "pa_h3", "relu", B, "a.L3")
    fwd(ac, 3, buf["pa_h3"], "a_out", "tanh", B, "a.L4")
    fwd(cr, 0, buf["bs"], "pc_h1", "relu", B, "c'.L1")
    fwd(cr, 1, torch.cat([buf["pc_h1"], buf["a_out"]], 1), "pc_h2", "relu",
        B, "c'.L2")
    fwd(cr, 2, buf["pc_h2"], "pc_h3", "relu", B, "c'.L3")
    fwd(cr, 3, buf["pc_h3"], "pq", "softmax", B, "c'.L4")
    # dX back through the critic
    _check_dx(cr, 3, buf["pd3"], buf["pc_h3"], buf["pd2"], "c'.L4 dX")
    _check_dx(cr, 2, buf["pd2"], buf["pc_h2"], buf["pdh1"], "c'.L3 dX")
    # the action slice is k_dx_narrow: plain fp32, unrounded operands
    l = cr.layers[1]
    dz, w = buf["pdh1"].double(), cr.w[1][l["in1"]:].double()
    _close(buf["pda"], dz @ w.t(), (l["out"] + 2) * U * (dz.abs() @ w.abs().t()),
           "c'.L2 dX (action slice, fp32)")
    # actor backward
    _check_dx(ac, 3, buf["adz"], buf["pa_h3"], buf["az3"], "a.L4 dX")
    _check_dx(ac, 2, buf["az3"], None, buf["az2"], "a.L3 dX")
    _check_dx(ac, 1, buf["az2"], buf["pa_h1"], buf["az1"], "a.L2 dX")
    g = phased["g_actor"]
    _check_dw(ac, g, 3, buf["adz"], buf["pa_h3"], None, B, "a.L4")
    _check_dw(ac, g, 2, buf["az3"], buf["pa_h2"], None, B, "a.L3")
    _check_dw(ac, g, 1, buf["az2"], buf["pa_h1"], None, B, "a.L2")
    _check_dw(ac, g, 0, buf["az1"], buf["bs"], None, B, "a.L1")


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
    return {n: eng.store_slab(n) for n in SLABS}


def _assert_slabs_equal(x, y, what):
    for n in SLABS:
        assert torch.equal(x[n].view(torch.int32), y[n].view(torch.int32)), \
            f"{what}: slab {n} differs"


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
