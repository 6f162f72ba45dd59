"""Adam and the target soft update, element by element, on every path.

k_adam_lerp, k_adam_lerp_clip (row-block and wide paths, and every split
step) and p_adam_lerp (inlined into the four k_step_persistent<CLIP, QR>
instantiations) are the only kernels that write the four parameter slabs.
Each of their four outputs (m', v', p', tgt') is compared with
tests/_oracles.py::adam_lerp_oracle, a float64 evaluation with the device's
float32 constants, teacher-forced stage by stage on the device's own stored
outputs and bounded elementwise by a count of float32 roundings (the bounds
are derived there; tests/test_adam_oracle.py shows on the CPU that they admit
the honest spellings and reject ten wrong ones).

Every engine has lr_actor = 2.5e-4 != lr_critic = 1e-3 and tau = 0.05, and the
targets are loaded DECOUPLED from the online nets (tgt = p + d), so a swapped
learning rate or a soft update that is skipped, reversed or taken toward the
old parameter moves an output by far more than its bound.  The slabs hold a
seeded normal bulk plus the repeating edge block of _oracles.ADAM_EDGES.

  a. k_adam_lerp on injected slabs: step_part(PH_*_APPLY) over five loaded
     slabs, t = 1 .. 2^24 + 1 through set_schedule.  Shapes: slabs of about 9k
     elements (less than one grid stride of 65536) and n_critic = 145971
     (three ragged strides; two ragged outer iterations of p_adam_lerp).
  b. k_adam_lerp_clip: the same with max_grad_norm = half the float64 norm of
     the injected gradient, scale from grad_stats(); and with a threshold that
     never binds, bitwise (a)'s result.
  c. p_adam_lerp through one persistent step(1), all four <CLIP, QR>: p, tgt,
     m, v and t injected, the gradient read back after the step (the slab
     keeps the raw gradient Adam consumed).
  d. the row-block (B = 300) and wide (B = 520) paths through a real step(1):
     launch_adam_lerp is reached with the right pointers and learning rates
     from enqueue_step_rowblock and enqueue_step_wide too.

Every case prints max err / bound per output before it asserts, and the worst
so far per (kernel, output): the figures of PARITY.md.

Not pinned: adam_t_actor and adam_t_critic cannot be made to differ through
the public API (set_schedule and the per-step tick move them together), so
which of the two counters a launch reads (`is_actor`) stays unchecked.
"""

import functools

import numpy as np
import pytest
import torch

import _engine_kit as kit
from _oracles import ADAM_EDGES, adam_fill, adam_lerp_oracle

pytestmark = pytest.mark.gpu

LR_ACTOR, LR_CRITIC, TAU = 2.5e-4, 1e-3, 0.05
LR = {"actor": LR_ACTOR, "critic": LR_CRITIC}
CAP, N_ROWS = 4096, 1024
NETS = ("critic", "actor")
OUT = ("m", "v", "p", "tgt")
T_LIST = [1, 2, 3, 7, 10, 100, 693, 1000, 10 ** 4, 10 ** 5, 2 ** 24 + 1]
T_STEP = [1, 2, 693, 10 ** 5]

SHAPES = {
    "small": dict(B=8, H=64, O=3, A=1, K=11),
    "big": dict(B=64, H=256, O=3, A=1, K=51),
    "rowblock": dict(B=300, H=128, O=3, A=1, K=51),
    "wide": dict(B=520, H=100, O=3, A=1, K=51),
}
N_CRITIC_BIG = 145971

# worst err / bound per (kernel, output), and the worst relative error of the
# step itself per kernel, in units of 2^-24
WORST = {}
STEP_REL = {}


def _slab_names(net):
    return {"p": net, "g": "g_" + net, "m": "m_" + net, "v": "v_" + net,
            "tgt": net + "_target"}


def _shape(name):
    return kit.Shape(**SHAPES[name])


@functools.lru_cache(maxsize=None)
def _rows(name):
    return kit.transitions(_shape(name), N_ROWS, seed=SHAPES[name]["B"])


@functools.lru_cache(maxsize=None)
def _net_params(name):
    """Freshly initialised online nets as slabs (read-only)."""
    a, _, cr, _ = kit.modules(_shape(name), seed=SHAPES[name]["B"])
    out = {"actor": kit.pack(a), "critic": kit.pack(cr)}
    for x in out.values():
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _engine(name, max_grad_norm=0.0, dist="categorical"):
    """One engine per configuration, shared by the cases: every case loads
    all the slabs it reads and sets the schedule itself.  One whole step first,
    so the sampled-batch buffers the PER write-back of PH_ACTOR_APPLY reads
    hold a real batch."""
    eng = kit.engine(_shape(name), capacity=CAP, tau=TAU, lr_actor=LR_ACTOR,
                     lr_critic=LR_CRITIC, max_grad_norm=max_grad_norm,
                     dist=dist)
    for net, p in _net_params(name).items():
        eng.load_slab(net, torch.from_numpy(p.copy()))
        eng.load_slab(net + "_target", torch.from_numpy(p.copy()))
    eng.ingest(*[torch.from_numpy(x) for x in _rows(name)])
    assert eng._persistent == (SHAPES[name]["B"] <= 256)
    eng.step(1)
    return eng


@functools.lru_cache(maxsize=None)
def _fill(name, net, real_p=False):
    """The five input slabs of one net (read-only) and the class vector."""
    n = _net_params(name)[net].size
    s, klass = adam_fill(n, seed=1000 * SHAPES[name]["B"] + (net == "actor"),
                         p=_net_params(name)[net] if real_p else None,
                         modest=real_p)
    for x in s.values():
        x.setflags(write=False)
    return s, klass


def _load(eng, net, s, keys):
    for k in keys:
        eng.load_slab(_slab_names(net)[k], torch.from_numpy(s[k].copy()))


def _read(eng, net, keys=OUT):
    return {k: eng.store_slab(_slab_names(net)[k]).numpy() for k in keys}


def _check(kernel, what, s, klass, out, t, lr, scale=1.0):
    """Print err / bound of the four outputs, then assert them."""
    ref = adam_lerp_oracle(s["p"], s["g"], s["m"], s["v"], s["tgt"], t, lr,
                           TAU, scale, got=out)
    fails = []
    for k in OUT:
        exp, bound = ref[k]
        err = np.abs(out[k].astype(np.float64) - exp)
        ratio = err / bound
        i = int(np.argmax(np.where(np.isnan(ratio), np.inf, ratio)))
        r = float(ratio[i])
        WORST[(kernel, k)] = max(WORST.get((kernel, k), 0.0), r) \
            if r == r else float("nan")
        cls = "bulk" if klass[i] < 0 else ADAM_EDGES[klass[i]][0]
        print(f"{what} t={t} {k}': max err/bound {r:.3f} at [{i}] ({cls}: "
              f"got {out[k][i]!r} want {exp[i]!r} bound {bound[i]:.3e})")
        if k == "p":
            # where the step dwarfs p the error is the step's own: a measure
            # of bc1 and sqrt(bc2) as the device formed them (the bound
            # allows E1 + E2 / 2, about 2000 * 2^-24 at t = 1)
            step = np.abs(s["p"].astype(np.float64) - exp)
            big = step > 16 * np.abs(s["p"])
            if big.any():
                rel = float((err[big] / step[big]).max()) / 2.0 ** -24
                STEP_REL[kernel] = max(STEP_REL.get(kernel, 0.0), rel)
                print(f"{what} t={t}: step relative error {rel:.2f} * 2^-24 "
                      f"(the rounding of p' included) over {int(big.sum())} "
                      f"elements with |step| > 16 |p|")
        bad = ~(err <= bound)
        if bad.any():
            names = sorted({("bulk" if c < 0 else ADAM_EDGES[c][0])
                            for c in set(klass[bad].tolist())})
            fails.append(f"{k}': {int(bad.sum())} of {bad.size} elements "
                         f"outside the bound, classes {names}")
    print("worst err/bound so far:",
          {f"{kn} {k}": round(v, 3) for (kn, k), v in sorted(WORST.items())})
    print("worst step relative error so far, in 2^-24:",
          {kn: round(v, 2) for kn, v in sorted(STEP_REL.items())})
    assert not fails, f"{what} t={t}: " + "; ".join(fails)


def _f64_norm(g):
    return float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))


def test_shapes_cover_the_strides():
    """The big critic slab is three ragged k_adam_lerp strides and two ragged
    outer iterations of p_adam_lerp; the small slabs are less than one."""
    n = _net_params("big")["critic"].size
    assert n == N_CRITIC_BIG
    assert 2 * 65536 < n < 3 * 65536 and 96 * 256 * 4 < n < 2 * 96 * 256 * 4
    for net in NETS:
        assert _net_params("small")[net].size < 65536 // 4
        s, klass = _fill("small", net)
        assert set(klass[klass >= 0]) == set(range(len(ADAM_EDGES)))
        assert np.abs(s["tgt"] - s["p"])[klass < 0].mean() > 0.05


# ---------------------------------------------------------------------------
# a. k_adam_lerp on injected slabs
# ---------------------------------------------------------------------------

def _apply(eng, net, s, t):
    """Load the five slabs, run the net's APPLY phase at Adam step t."""
    _load(eng, net, s, ("p", "g", "m", "v", "tgt"))
    eng.set_schedule(t - 1)
    eng.step_part(eng.PH_CRITIC_APPLY if net == "critic"
                  else eng.PH_ACTOR_APPLY)
    out = _read(eng, net)
    g_after = eng.store_slab("g_" + net).numpy()
    assert np.array_equal(g_after.view(np.uint32), s["g"].view(np.uint32)), \
        f"{net}: the gradient slab was modified"
    if net == "actor":          # the step's last phase ticks the counters
        assert eng.counters()["adam_t_actor"] == t
    return out


def _assert_untouched_class(s, klass, out, what):
    """g = m = v = 0: the step is exactly zero and p' is p bitwise."""
    at = klass == 0
    assert at.any()
    assert np.array_equal(out["p"][at].view(np.uint32),
                          s["p"][at].view(np.uint32)), what


@pytest.mark.parametrize("t", T_LIST)
@pytest.mark.parametrize("name", ["small", "big"])
def test_k_adam_lerp_on_injected_slabs(name, t):
    eng = _engine(name)
    for net in NETS:
        s, klass = _fill(name, net)
        out = _apply(eng, net, s, t)
        what = f"k_adam_lerp {name} {net} n={s['p'].size}"
        _check("k_adam_lerp", what, s, klass, out, t, LR[net])
        _assert_untouched_class(s, klass, out, what)


# ---------------------------------------------------------------------------
# b. k_adam_lerp_clip
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("t", T_LIST)
@pytest.mark.parametrize("name", ["small", "big"])
def test_k_adam_lerp_clip_on_injected_slabs(name, t):
    """One engine per net, its threshold half the float64 norm of that net's
    injected gradient; Adam must consume float32(scale) * g, scale as
    grad_stats() reports it (pinned bitwise in tests/test_gpu_grad_clip.py)."""
    for net in NETS:
        s, klass = _fill(name, net)
        norm = _f64_norm(s["g"])
        eng = _engine(name, max_grad_norm=0.5 * norm)
        out = _apply(eng, net, s, t)
        st = eng.grad_stats()
        scale = st["scale_" + net]
        what = f"k_adam_lerp_clip {name} {net} n={s['p'].size}"
        print(f"{what}: norm {st['norm_' + net]!r} numpy {norm!r} scale "
              f"{scale!r}")
        assert abs(st["norm_" + net] - norm) <= 1e-10 * norm
        assert 0.49 < scale < 0.51
        _check("k_adam_lerp_clip", what, s, klass, out, t, LR[net], scale)
        _assert_untouched_class(s, klass, out, what)


@pytest.mark.parametrize("t", T_LIST)
@pytest.mark.parametrize("name", ["small", "big"])
def test_clip_that_never_binds_is_bitwise_the_plain_kernel(name, t):
    plain, clip = _engine(name), _engine(name, max_grad_norm=1e30)
    for net in NETS:
        s, _ = _fill(name, net)
        a, b = _apply(plain, net, s, t), _apply(clip, net, s, t)
        assert clip.grad_stats()["scale_" + net] == 1.0
        for k in OUT:
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), \
                f"{name} {net} t={t}: {k}' differs at scale 1.0"


# ---------------------------------------------------------------------------
# c, d. through a whole step: the gradient is the engine's own
# ---------------------------------------------------------------------------

def _whole_step(kernel, name, t, max_grad_norm=0.0, dist="categorical"):
    eng = _engine(name, max_grad_norm, dist)
    fills = {net: _fill(name, net, real_p=True) for net in NETS}
    for net in NETS:
        _load(eng, net, fills[net][0], ("p", "m", "v", "tgt"))
    eng.set_schedule(t - 1)
    eng.step(1)
    assert eng.counters()["adam_t_actor"] == t
    assert eng.counters()["adam_t_critic"] == t
    st = eng.grad_stats()
    for net in NETS:
        s, klass = fills[net]
        out = _read(eng, net)
        s = dict(s, g=eng.store_slab("g_" + net).numpy())
        assert np.isfinite(s["g"]).all() and s["g"].any()
        scale = 1.0
        if max_grad_norm:
            scale = st["scale_" + net]
            print(f"{kernel} {name} {net}: norm {st['norm_' + net]!r} scale "
                  f"{scale!r}")
            assert 0.0 < scale < 1.0, "the threshold was meant to bind"
        _check(kernel, f"{kernel} {name} {net} n={s['p'].size}", s, klass,
               out, t, LR[net], scale)


@pytest.mark.parametrize("t", T_STEP)
@pytest.mark.parametrize("name", ["small", "big"])
def test_p_adam_lerp_plain(name, t):
    _whole_step("p_adam_lerp<0,0>", name, t)


# a threshold far below any gradient norm these steps produce: it binds
CLIP_C = 1e-4


@pytest.mark.parametrize("t", T_STEP)
@pytest.mark.parametrize("clip,dist", [(CLIP_C, "categorical"),
                                       (0.0, "quantile"),
                                       (CLIP_C, "quantile")])
def test_p_adam_lerp_clip_and_quantile(clip, dist, t):
    kernel = f"p_adam_lerp<{int(clip > 0)},{int(dist == 'quantile')}>"
    _whole_step(kernel, "small", t, clip, dist)


@pytest.mark.parametrize("t", [1, 693])
@pytest.mark.parametrize("name", ["rowblock", "wide"])
def test_rowblock_and_wide_reach_adam_through_a_real_step(name, t):
    _whole_step(f"k_adam_lerp ({name} step)", name, t)
