"""GEMM-by-GEMM harness of the wide train step, shared by
test_gpu_wide_bf16.py (bf16 operands) and test_gpu_wide.py (fp32 operands).

Every GEMM is checked on its own, teacher-forced: the expected value is built
from the engine's OWN fp32 input buffers of that GEMM, so a rounding flip
upstream cannot leak into the comparison,

    expected = rnd(a) @ rnd(b) (+ fp32 bias)          in float64

with rnd the operand rounding of the engine's gemm_precision: `bf` (to bf16,
round-to-nearest-even) or `exact` (the identity, fp32 operands).  Products of
two bf16 values are exact in fp32; products of two fp32 values are rounded
once, which the fused multiply-add folds into the accumulation step.  Either
way the only error left is the fp32 accumulation, bounded for ANY summation
order by

    (K + ksplit + 2) * 2^-23 * (|rnd(a)| @ |rnd(b)| + |bias|)

elementwise (K the summed dimension, ksplit the split-K factor of that
launch; unit roundoff 2^-23 rather than 2^-24 also covers adds inside the
MFMA that do not round to nearest).  ReLU and the 0/1 ReLU mask do not grow
the bound; outputs behind tanh or softmax use the 5e-5 atol of
tests/test_gpu_wide.py.
"""

import torch

import _engine_kit as kit
from _engine_kit import SLABS

LR = 1e-4
N_ROWS = 4096
U = 2.0 ** -23

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


def _shape(c, precision="fp32", batch=None):
    return kit.Shape(batch or c["B"], c["H"], c["O"], c["A"], c["K"],
                     precision=precision)


def _modules(c, seed=5):
    return kit.modules(_shape(c), seed)


def _rows(c, seed=7):
    return kit.transitions(_shape(c), N_ROWS, seed)


def _engine(c, precision="bf16", mods=None, rows=None, seed=11, batch=None):
    return kit.engine(_shape(c, precision, batch), mods or _modules(c),
                      rows or _rows(c), capacity=8192, seed=seed)


# ---------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------

def bf(x):
    return x.to(torch.bfloat16).to(torch.float64)


def exact(x):
    return x.to(torch.float64)


ROUNDING = {"bf16": bf, "fp32": exact}

# largest error / bound seen per GEMM kind, for the record in PARITY.md
WORST = {}


def _gemm(a, b, k, ksplit, bias=None, rnd=bf):
    """(expected, bound) of rnd(a) @ rnd(b) + bias, float64."""
    a, b = rnd(a), rnd(b)
    exp = a @ b
    mag = a.abs() @ b.abs()
    if bias is not None:
        exp = exp + bias.to(torch.float64)
        mag = mag + bias.to(torch.float64).abs()
    return exp, (k + ksplit + 2) * U * mag


def _close(got, exp, bound, what, kind=None):
    err = (got.to(torch.float64) - exp).abs()
    worst = float((err - bound).max())
    ratio = float((err / bound.clamp_min(1e-300)).max())
    if kind is not None:
        WORST[kind] = max(WORST.get(kind, 0.0), ratio)
    print(f"{what}: max err {float(err.max()):.3e}, "
          f"max bound {float(bound.max()):.3e}, max err/bound {ratio:.3f}")
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


class Checks:
    """The three per-GEMM checks for one operand rounding."""

    def __init__(self, precision):
        self.precision = precision
        self.rnd = ROUNDING[precision]

    def fwd(self, buf, net, i, x, got, act, B, what):
        l = net.layers[i]
        n_in = l["in1"] + l["in2"]
        ks = _ks_head(B, n_in) if l["out"] <= 64 else 1
        exp, bound = _gemm(x, net.w[i], n_in, ks, net.b[i], rnd=self.rnd)
        kind = (self.precision, "fwd")
        if act == "relu":
            exp = exp.clamp_min(0)
        elif act == "tanh":
            exp, bound, kind = exp.tanh(), torch.full_like(exp, 5e-5), None
        elif act == "softmax":
            exp, bound, kind = exp.softmax(1), torch.full_like(exp, 5e-5), None
        _close(buf[got], exp, bound, what, kind)

    def dx(self, net, i, dz, mask_h, got, what):
        """dx1 = (dz @ W[:in1]^T) * relu'(mask_h)."""
        l = net.layers[i]
        exp, bound = _gemm(dz, net.w[i][:l["in1"]].t(), l["out"], 1,
                           rnd=self.rnd)
        if mask_h is not None:
            m = (mask_h > 0).to(torch.float64)
            exp, bound = exp * m, bound * m
        _close(got, exp, bound, what, (self.precision, "dx"))

    def dw(self, net, g, i, dz, x1, x2, B, what):
        """The layer's block of the gradient slab: dWt (per input block, as
        the engine runs it) and db."""
        l = net.layers[i]
        gnet = Net(g, net.layers)
        lo = 0
        for x in (x1, x2):
            if x is None:
                continue
            n = x.shape[1]
            ks = _ks_dw(B, n, l["out"])
            exp, bound = _gemm(x.t(), dz, B, ks, rnd=self.rnd)
            _close(gnet.w[i][lo:lo + n], exp, bound,
                   f"{what} dW[{lo}:{lo + n}]", (self.precision, "dw"))
            lo += n
        ks = _ks_dw(B, l["in1"], l["out"])
        exp, bound = _gemm(torch.ones(1, B), dz, B, ks, rnd=self.rnd)
        _close(gnet.b[i], exp[0], bound[0], f"{what} db",
               (self.precision, "db"))


# ---------------------------------------------------------------------------
# teacher-forced, GEMM by GEMM
# ---------------------------------------------------------------------------

def run_phased(name, precision):
    """One engine of config `name`, stepped phase by phase; every buffer and
    slab read after the phase that wrote it."""
    c = CONFIGS[name]
    eng = _engine(c, precision)
    info = eng.info()
    assert info["gemm_precision"] == precision
    st = {"cfg": c, "name": name, "info": info, "precision": precision}
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


def check_critic_phase(phased):
    c, buf, info = phased["cfg"], phased["critic"], phased["info"]
    ck = Checks(phased["precision"])
    B = c["B"]
    s0 = phased["slabs0"]
    at = Net(s0["actor_target"], info["actor_layers"])
    ct = Net(s0["critic_target"], info["critic_layers"])
    cr = Net(s0["critic"], info["critic_layers"])
    cat = lambda a, b: torch.cat([buf[a], buf[b]], 1)
    fwd = lambda *a: ck.fwd(buf, *a)
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
    ck.dx(cr, 3, buf["dlog"], buf["c_h3"], buf["d3"], "c.L4 dX")
    ck.dx(cr, 2, buf["d3"], buf["c_h2"], buf["d2"], "c.L3 dX")
    ck.dx(cr, 1, buf["d2"], buf["c_h1"], buf["d1"], "c.L2 dX")
    g = phased["g_critic"]
    ck.dw(cr, g, 3, buf["dlog"], buf["c_h3"], None, B, "c.L4")
    ck.dw(cr, g, 2, buf["d3"], buf["c_h2"], None, B, "c.L3")
    ck.dw(cr, g, 1, buf["d2"], buf["c_h1"], buf["ba"], B, "c.L2")
    ck.dw(cr, g, 0, buf["d1"], buf["bs"], None, B, "c.L1")


def check_actor_phase(phased):
    c, buf, info = phased["cfg"], phased["actor"], phased["info"]
    ck = Checks(phased["precision"])
    B = c["B"]
    ac = Net(phased["slabs0"]["actor"], info["actor_layers"])
    cr = Net(phased["p_critic1"], info["critic_layers"])  # after its Adam
    fwd = lambda *a: ck.fwd(buf, *a)
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
    ck.dx(cr, 3, buf["pd3"], buf["pc_h3"], buf["pd2"], "c'.L4 dX")
    ck.dx(cr, 2, buf["pd2"], buf["pc_h2"], buf["pdh1"], "c'.L3 dX")
    # the action slice is k_dx_narrow: plain fp32, unrounded operands
    l = cr.layers[1]
    dz, w = buf["pdh1"].double(), cr.w[1][l["in1"]:].double()
    _close(buf["pda"], dz @ w.t(), (l["out"] + 2) * U * (dz.abs() @ w.abs().t()),
           "c'.L2 dX (action slice, fp32)")
    # actor backward
    ck.dx(ac, 3, buf["adz"], buf["pa_h3"], buf["az3"], "a.L4 dX")
    ck.dx(ac, 2, buf["az3"], None, buf["az2"], "a.L3 dX")
    ck.dx(ac, 1, buf["az2"], buf["pa_h1"], buf["az1"], "a.L2 dX")
    g = phased["g_actor"]
    ck.dw(ac, g, 3, buf["adz"], buf["pa_h3"], None, B, "a.L4")
    ck.dw(ac, g, 2, buf["az3"], buf["pa_h2"], None, B, "a.L3")
    ck.dw(ac, g, 1, buf["az2"], buf["pa_h1"], None, B, "a.L2")
    ck.dw(ac, g, 0, buf["az1"], buf["bs"], None, B, "a.L1")
    print("max err/bound so far:",
          {f"{p} {k}": round(v, 4) for (p, k), v in sorted(WORST.items())})
