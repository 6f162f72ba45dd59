"""The bounds of tests/_oracles.py::adam_lerp_oracle are sound and have teeth
(CPU only: numpy float32 spellings of the element update stand in for the
kernels, so nobody has to build a broken kernel for the GPU).

Sound: the unfused spelling of k_adam_lerp and two fused ones (p_adam_lerp's,
with the second moment and the soft update contracted into an fma, and one
that fuses the first moment too) stay inside the bounds at every element of
the edge vector and every t of the GPU test's list, with bc = 1 - b^t formed
in float32 from the exact b^t and from b^t at both ends of the error the
bounds allow it (4 * 2^-24, see _perturbed_bc).

Teeth: each wrong spelling leaves the bound on at least 1% of the bulk
elements.  Mutations that do not involve the bias correction must do so at
every t; the bias-correction ones at t = 1, 2, 3 (at large t both bc terms
are 1 and dropping or exchanging them changes nothing).  "One element left
untouched" is a single element and must be flagged itself.

An fma is emulated as float32(double(a) * double(b) + double(c)): the product
is exact in double, so this differs from a true fma only by double rounding.
"""

import itertools

import numpy as np
import pytest

from _oracles import (ADAM_EDGES, ADAM_POW_ERR, adam_bc64, adam_fill,
                      adam_lerp_oracle)

f32, f64 = np.float32, np.float64
T_LIST = [1, 2, 3, 7, 10, 100, 693, 1000, 10 ** 4, 10 ** 5, 2 ** 24 + 1]
LR_ACTOR, LR_CRITIC, TAU = 2.5e-4, 1e-3, 0.05
N = 20000
B1, B2, EPS = f32(0.9), f32(0.999), f32(1e-8)


def _fma(a, b, c):
    return (np.asarray(a, f64) * np.asarray(b, f64)
            + np.asarray(c, f64)).astype(f32)


def _perturbed_bc(t, s1, s2):
    """float32 (bc1, bc2) from b^t off by s * ADAM_POW_ERR (s in -1, 0, 1):
    the float32 value furthest from the exact b^t that is still within the
    error the oracle assumes of the device's pow."""
    out = []
    for b, s in ((B1, s1), (B2, s2)):
        exact = f64(b) ** f64(t)
        x = f32(exact + s * ADAM_POW_ERR)
        if abs(f64(x) - exact) > ADAM_POW_ERR:
            x = np.nextafter(x, f32(exact), dtype=f32)
        assert abs(f64(x) - exact) <= ADAM_POW_ERR
        out.append(f32(f32(1) - x))
    return out


def update(s, bc1, bc2, lr, tau, scale=None, fuse=(), mut=None):
    """float32 element update.  fuse: subset of {"m", "v", "v2", "t"} (v: the
    gs^2 product fused, v2: the b2 v product fused).  mut: a wrong spelling."""
    lr, tau = f32(lr), f32(tau)
    p, g, m, v, tgt = (s[k] for k in ("p", "g", "m", "v", "tgt"))
    gs = g if scale is None else f32(scale) * g
    if mut == "scale_twice":
        gs = f32(scale) * gs
    if mut == "bc_swapped":
        bc1, bc2 = bc2, bc1
    omb1, omb2 = f32(1) - B1, f32(1) - B2
    mi = _fma(omb1, gs, B1 * m) if "m" in fuse else B1 * m + omb1 * gs
    if "v" in fuse:
        vi = _fma(omb2 * gs, gs, B2 * v)
    elif "v2" in fuse:
        vi = _fma(B2, v, omb2 * gs * gs)
    else:
        vi = B2 * v + omb2 * gs * gs
    if mut == "eps_in_sqrt":
        den = np.sqrt(vi / bc2 + EPS)
    elif mut == "no_bc2":
        den = np.sqrt(vi) + EPS
    elif mut == "sqrt_over_bc2":
        den = np.sqrt(vi) / bc2 + EPS
    else:
        den = np.sqrt(vi / bc2) + EPS
    pn = p - lr * (mi / bc1) / den
    src = p if mut == "lerp_old_p" else pn
    d = tgt - src if mut == "lerp_sign" else src - tgt
    tn = _fma(tau, d, tgt) if "t" in fuse else tgt + tau * d
    if mut == "lerp_skipped":
        tn = tgt.copy()
    out = {"m": mi.astype(f32), "v": vi.astype(f32), "p": pn.astype(f32),
           "tgt": tn.astype(f32)}
    if mut == "one_untouched":
        for k in out:
            out[k][UNTOUCHED] = s[k][UNTOUCHED]
    return out


def outside(s, out, t, lr, tau, scale=1.0):
    """Per element: some output is not within the oracle's bound."""
    ref = adam_lerp_oracle(s["p"], s["g"], s["m"], s["v"], s["tgt"], t, lr,
                           tau, scale, got=out)
    bad = np.zeros(s["p"].shape, bool)
    ratio = {}
    for k, (exp, bound) in ref.items():
        err = np.abs(out[k].astype(f64) - exp)
        bad |= ~(err <= bound)
        ratio[k] = float((err / bound).max())
    return bad, ratio


SLABS, KLASS = adam_fill(N, seed=1)
BULK = KLASS < 0
UNTOUCHED = int(np.flatnonzero(BULK)[137])
HONEST = {"unfused": (), "fused v, tgt": ("v", "t"),
          "fused m, v, tgt": ("m", "v2", "t")}


def test_the_fill_holds_every_class_and_decoupled_targets():
    assert set(KLASS[KLASS >= 0]) == set(range(len(ADAM_EDGES)))
    assert BULK.mean() > 0.7
    assert np.abs(SLABS["tgt"] - SLABS["p"])[BULK].mean() > 0.05
    for k in SLABS:
        assert SLABS[k].dtype == f32 and np.isfinite(SLABS[k]).all()
    assert (SLABS["v"] >= 0).all()


@pytest.mark.parametrize("scale", [None, 0.37])
@pytest.mark.parametrize("name", list(HONEST))
def test_honest_spellings_stay_inside_the_bounds(name, scale):
    worst = {}
    for t in T_LIST:
        ex1, ex2 = adam_bc64(t)
        for s1, s2 in itertools.product((0, 1, -1), repeat=2):
            bc1, bc2 = _perturbed_bc(t, s1, s2)
            for lr in (LR_ACTOR, LR_CRITIC):
                out = update(SLABS, bc1, bc2, lr, TAU, scale, HONEST[name])
                bad, ratio = outside(SLABS, out, t, lr, TAU,
                                     1.0 if scale is None else scale)
                for k, r in ratio.items():
                    worst[k] = max(worst.get(k, 0.0), r)
                assert not bad.any(), (
                    f"{name} t={t} bc error ({s1}, {s2}) lr={lr}: classes "
                    f"{sorted(set(KLASS[bad]))} leave the bound, max "
                    f"err/bound {ratio}")
        print(f"{name} scale={scale} t={t}: bc1 {ex1:.6g} bc2 {ex2:.6g} "
              f"accepted; worst err/bound so far "
              f"{ {k: round(r, 3) for k, r in worst.items()} }")
    assert all(0 < r <= 1 for r in worst.values())


def test_zero_gradient_and_moments_leave_p_bitwise():
    at = KLASS == 0
    for t in T_LIST:
        bc1, bc2 = _perturbed_bc(t, 0, 0)
        out = update(SLABS, bc1, bc2, LR_CRITIC, TAU)
        assert np.array_equal(out["p"][at], SLABS["p"][at])


# mutation -> must be rejected at every t (True) or at t <= 3 (False)
MUTATIONS = {"lerp_skipped": True, "lerp_old_p": True, "lerp_sign": True,
             "eps_in_sqrt": True, "no_bc2": False, "sqrt_over_bc2": False,
             "bc_swapped": False, "lr_actor_for_critic": True,
             "scale_twice": True}


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_wrong_spellings_leave_the_bound(mut):
    scale = 0.37 if mut == "scale_twice" else None
    for t in T_LIST:
        bc1, bc2 = _perturbed_bc(t, 0, 0)
        lr = LR_ACTOR if mut == "lr_actor_for_critic" else LR_CRITIC
        for fuse in HONEST.values():
            out = update(SLABS, bc1, bc2, lr, TAU, scale, fuse, mut)
            bad, _ = outside(SLABS, out, t, LR_CRITIC, TAU,
                             1.0 if scale is None else scale)
            frac = bad[BULK].mean()
            print(f"{mut} t={t} fuse={fuse}: {100 * frac:.1f}% of the bulk, "
                  f"{100 * bad[~BULK].mean():.1f}% of the edges rejected")
            if MUTATIONS[mut] or t <= 3:
                assert frac >= 0.01, (mut, t, fuse, frac)


def test_one_untouched_element_is_rejected():
    for t in T_LIST:
        bc1, bc2 = _perturbed_bc(t, 0, 0)
        out = update(SLABS, bc1, bc2, LR_CRITIC, TAU, mut="one_untouched")
        bad, _ = outside(SLABS, out, t, LR_CRITIC, TAU)
        print(f"one_untouched t={t}: rejected {np.flatnonzero(bad).tolist()}")
        assert np.flatnonzero(bad).tolist() == [UNTOUCHED]


def test_eps_dominated_class_separates_every_eps_placement():
    """m = 1e-3, v = 1e-20, g = 0: the step is about 1e5 * lr, and moving eps
    under the square root moves it far outside the bound at every t."""
    at = (KLASS == [n for n, *_ in ADAM_EDGES].index("eps+")) | \
         (KLASS == [n for n, *_ in ADAM_EDGES].index("eps-"))
    for t in T_LIST:
        bc1, bc2 = _perturbed_bc(t, 0, 0)
        good = update(SLABS, bc1, bc2, LR_CRITIC, TAU)
        assert (np.abs(good["p"] - SLABS["p"])[at] > 1e4 * LR_CRITIC).all()
        out = update(SLABS, bc1, bc2, LR_CRITIC, TAU, mut="eps_in_sqrt")
        bad, _ = outside(SLABS, out, t, LR_CRITIC, TAU)
        assert bad[at].all()
