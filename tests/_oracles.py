"""Plain numpy oracles for the fused engine's PER sampling, C51 projection,
replay ring, rollout noise streams and fused Adam + target soft update (shared
by the CPU and GPU tests; not a conftest).

Everything here is written for clarity, not speed: python loops, float64
mass arithmetic.  Where the engine's result depends on a float32 rounding
(the philox -> (0,1] map, the beta schedule, the projection's bin position)
that rounding is reproduced so the *discrete* choices (leaf, bin) are the
engine's own and only the continuous arithmetic is higher precision.
"""

from __future__ import annotations

import numpy as np

_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF


def philox4x32_10_raw(ctr, key):
    """philox4x32-10 on a 4-word counter and 2-word key (Salmon et al.,
    'Parallel random numbers: as easy as 1, 2, 3', SC'11)."""
    c0, c1, c2, c3 = (int(x) & _MASK for x in ctr)
    k0, k1 = (int(x) & _MASK for x in key)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0, p1 & _MASK,
                          (p0 >> 32) ^ c3 ^ k1, p0 & _MASK)
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def philox4x32_10(seed, ctr_hi, ctr_lo):
    """The engine's calling convention: 64-bit seed -> key, 64-bit ctr_lo ->
    counter words 0,1 and 64-bit ctr_hi -> counter words 2,3."""
    seed, ctr_hi, ctr_lo = int(seed), int(ctr_hi), int(ctr_lo)
    return philox4x32_10_raw(
        (ctr_lo, ctr_lo >> 32, ctr_hi, ctr_hi >> 32), (seed, seed >> 32))


def u01(x):
    """uint32 -> (0, 1] exactly as the kernel rounds it: cast to float32,
    add 1, multiply by 2^-32 (as the float32 literal), all in float32."""
    f = np.float32(np.uint32(int(x) & _MASK))
    return np.float32(np.float32(f + np.float32(1.0))
                      * np.float32(2.3283064e-10))


def probe_mass(seed, epoch, probe, total):
    """The sum-tree mass probe `probe` of step-epoch `epoch` descends with."""
    return float(u01(philox4x32_10(seed, epoch, probe)[0])) * float(total)


def uniform_index(seed, epoch, probe, n):
    """The uniform replay draw (tests/test_uniform_oracle.py): the first two
    words of the PER probe's stream as a 64-bit x, slot floor(x * n / 2^64)."""
    w = philox4x32_10(seed, epoch, probe)
    x = (w[0] << 32) | w[1]
    return (x * int(n)) >> 64


def uniform_batch(seed, epoch, B, n):
    return np.array([uniform_index(seed, epoch, i, n) for i in range(B)],
                    np.int64)


def build_trees(leaf_pri, tree_cap):
    """Binary-heap sum and min trees (node n has children 2n, 2n+1; leaves at
    [tree_cap, 2*tree_cap)) over `leaf_pri`, built bottom-up in float64 so
    every parent is bitwise the sum / min of its two children.  Unoccupied
    leaves hold what a fresh engine holds: 0 in the sum tree, +inf in the
    min tree (slot 0 is unused and keeps the same fill)."""
    leaf_pri = np.asarray(leaf_pri, np.float64)
    n = leaf_pri.shape[0]
    assert n <= tree_cap and tree_cap & (tree_cap - 1) == 0
    st = np.zeros(2 * tree_cap, np.float64)
    mt = np.full(2 * tree_cap, np.inf, np.float64)
    st[tree_cap:tree_cap + n] = leaf_pri
    mt[tree_cap:tree_cap + n] = leaf_pri
    for node in range(tree_cap - 1, 0, -1):
        st[node] = st[2 * node] + st[2 * node + 1]
        mt[node] = min(mt[2 * node], mt[2 * node + 1])
    return st, mt


def descend(sum_tree, tree_cap, mass, size):
    """The specification of a PER draw: plain binary descent.  Go left if
    mass <= left child, else subtract it and go right; a leaf past the
    occupied range (fp round-off at the top) snaps to size-1."""
    node = 1
    mass = float(mass)
    while node < tree_cap:
        left = float(sum_tree[2 * node])
        if mass <= left:
            node = 2 * node
        else:
            mass -= left
            node = 2 * node + 1
    idx = node - tree_cap
    return size - 1 if idx >= size else idx


def per_beta(beta0, beta_iters, beta_t):
    """float32 beta schedule as the sampling kernels compute it."""
    frac = min(np.float32(np.float64(beta_t)
                          / np.float64(np.float32(beta_iters))),
               np.float32(1.0))
    return np.float32(np.float32(beta0)
                      + np.float32(frac * np.float32(np.float32(1.0)
                                                     - np.float32(beta0))))


def is_weights(sum_tree, min_tree, idx, size, beta0, beta_iters, beta_t):
    """w_i = ((p_i/total) * N)^-beta / max_w, max_w = ((p_min/total)*N)^-beta
    (float64 throughout; beta is the float32 schedule value)."""
    tree_cap = len(sum_tree) // 2
    beta = float(per_beta(beta0, beta_iters, beta_t))
    total = float(sum_tree[1])
    idx = np.asarray(idx, np.int64)
    p = np.asarray(sum_tree, np.float64)[tree_cap + idx] / total
    p_min = float(min_tree[1]) / total
    max_w = (p_min * size) ** (-beta)
    return (p * size) ** (-beta) / max_w


def project64(p, r, d, v_min, v_max, gamma_n):
    """C51 projection, per row and per atom, masses in float64.

    The bin position b of each shifted atom is taken from float32 arithmetic
    (the values the kernel sees), capped at K-1, and only then split in
    float64 — so the bin choice is the kernel's and the oracle adds no
    bin-flip noise of its own.  Equal-bin rule: when b is integral, all of
    the atom's mass goes to bin b."""
    f = np.float32
    p = np.asarray(p, np.float64)
    r = np.asarray(r, np.float32).ravel()
    d = np.asarray(d, np.float32).ravel()
    B, K = p.shape
    v_min, v_max, gamma_n = f(v_min), f(v_max), f(gamma_n)
    delta = f(f(v_max - v_min) / f(K - 1))
    m = np.zeros((B, K), np.float64)
    for i in range(B):
        g = f(gamma_n * f(f(1.0) - d[i]))
        for j in range(K):
            z = f(v_min + f(f(j) * delta))
            tz = f(r[i] + f(g * z))
            tz = min(v_max, max(v_min, tz))
            b = min(f(f(tz - v_min) / delta), f(K - 1))
            lo, hi = int(np.floor(b)), int(np.ceil(b))
            if lo == hi:
                m[i, lo] += p[i, j]
            else:
                m[i, lo] += p[i, j] * (hi - float(b))
                m[i, hi] += p[i, j] * (float(b) - lo)
    return m


# ---------------------------------------------------------------------------
# replay write side: the ring, and the rollout's philox streams
# ---------------------------------------------------------------------------

class RingOracle:
    """The on-HBM replay as a plain numpy ring: rows are written one at a
    time at `pos`, so on a duplicate slot the last write wins; each new row's
    tree leaf is `leaf` (float64)."""

    def __init__(self, capacity, tree_cap):
        assert capacity <= tree_cap
        self.capacity, self.tree_cap = int(capacity), int(tree_cap)
        self.size = self.pos = 0
        self.rows = None
        self.leaves = np.zeros(self.capacity, np.float64)

    def add(self, s, a, r, s2, d, leaf=1.0):
        s, a, s2 = (np.asarray(x, np.float32) for x in (s, a, s2))
        r = np.asarray(r, np.float32).ravel()
        d = np.asarray(d, np.float32).ravel()
        T = len(r)
        s, a, s2 = s.reshape(T, -1), a.reshape(T, -1), s2.reshape(T, -1)
        if self.rows is None:
            c = self.capacity
            self.rows = dict(s=np.zeros((c, s.shape[1]), np.float32),
                             a=np.zeros((c, a.shape[1]), np.float32),
                             r=np.zeros(c, np.float32),
                             s2=np.zeros((c, s.shape[1]), np.float32),
                             d=np.zeros(c, np.float32))
        for t in range(T):
            i = self.pos
            self.rows["s"][i], self.rows["a"][i] = s[t], a[t]
            self.rows["r"][i], self.rows["d"][i] = r[t], d[t]
            self.rows["s2"][i] = s2[t]
            self.leaves[i] = leaf
            self.pos = (i + 1) % self.capacity
            self.size = min(self.size + 1, self.capacity)

    def occupied(self):
        """(s, a, r, s2, d) over rows [0, size)."""
        return tuple(self.rows[k][:self.size]
                     for k in ("s", "a", "r", "s2", "d"))

    def trees(self):
        return build_trees(self.leaves[:self.size], self.tree_cap)


def n01(a, b):
    """The rollout kernel's Box-Muller on two philox words: the uniforms are
    the kernel's float32 u01, the transcendental part is float64."""
    u1 = max(float(u01(a)), 1e-12)
    u2 = float(u01(b))
    return float(np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2))


def roll_noise_words(seed, ep, tick, env):
    """Philox words of env `env`'s exploration noise at `tick` of rollout
    episode `ep` (the first episode after rollout_alloc is ep = 1)."""
    return philox4x32_10(int(seed) ^ 0x2F01E, (int(ep) << 20) | (tick + 2),
                         env)


def roll_reset_state(seed, ep, env):
    """(th, thdot) the device reset gives env `env` at episode `ep`, in the
    kernel's float32 arithmetic."""
    v = philox4x32_10(int(seed) ^ 0xD011E, (int(ep) << 20) | 1, env)
    f = np.float32
    th = f(f(f(2.0) * u01(v[0]) - f(1.0)) * f(3.14159265358979))
    td = f(f(2.0) * u01(v[1]) - f(1.0))
    return th, td


def cpu_rollout(net, th0, td0, M, n_steps, horizon, gamma=0.99):
    """Oracle: VectorPendulum + VecNStep with the SAME start state and a
    noiseless policy; returns transitions in the device emit order
    (tick-major, env-minor)."""
    import torch
    from d4pg_amd.envs.vector import VecNStep, VectorPendulum
    env = VectorPendulum(M, seed=0, horizon=horizon)
    env.th = np.asarray(th0, np.float64).copy()
    env.thdot = np.asarray(td0, np.float64).copy()
    env.t = 0
    fold = VecNStep(M, 3, 1, n_steps, gamma)
    obs = env._obs()
    outs = []
    with torch.no_grad():
        for t in range(horizon):
            a = net(torch.from_numpy(obs)).numpy()
            a = np.clip(a, -1.0, 1.0).astype(np.float32)
            obs2, r, done = env.step(a)
            out = fold.push(obs, a, r, obs2, done)
            if out is not None:
                outs.append(out)
            obs = obs2
    return [np.concatenate([o[i] for o in outs]) for i in range(5)]


# ---------------------------------------------------------------------------
# edge-case reward/done rows for the projection tests
# ---------------------------------------------------------------------------

N_CATEGORIES = 8


def edge_rows(n, K, v_min, v_max, seed=0):
    """n (reward, done) rows whose category is `index % 8`:
      0  r far above v_max, done      1  r far above v_max, not done
      2  r far below v_min            3  done, r = float32(v_min + j*delta)
      4  done, r = v_min exactly         for j cycling over 0, 1, K//2, K-1
      5  done, r = v_max exactly      6  interior, not done
      7  interior, done
    """
    f = np.float32
    rng = np.random.default_rng(seed)
    delta = f(f(f(v_max) - f(v_min)) / f(K - 1))
    span = float(v_max) - float(v_min)
    js = [0, 1, K // 2, K - 1]
    r = np.zeros(n, np.float32)
    d = np.zeros(n, np.float32)
    for i in range(n):
        c = i % N_CATEGORIES
        if c == 0:
            r[i], d[i] = v_max + 10.0 * span, 1.0
        elif c == 1:
            r[i], d[i] = v_max + 10.0 * span, 0.0
        elif c == 2:
            r[i], d[i] = v_min - 10.0 * span, 0.0
        elif c == 3:
            j = js[(i // N_CATEGORIES) % 4]
            r[i], d[i] = f(f(v_min) + f(f(j) * delta)), 1.0
        elif c == 4:
            r[i], d[i] = v_min, 1.0
        elif c == 5:
            r[i], d[i] = v_max, 1.0
        elif c == 6:
            r[i], d[i] = rng.uniform(0.1 * span, 0.3 * span), 0.0
            r[i] = f(r[i] - f(0.35 * span))    # straddles some clamping
        else:
            r[i], d[i] = rng.uniform(v_min + 0.05 * span,
                                     v_max - 0.05 * span), 1.0
    return r, d


# ---------------------------------------------------------------------------
# fused Adam + target soft update, element by element
# ---------------------------------------------------------------------------

ADAM_U = 2.0 ** -23          # the unit of tests/_wide_gemm.py
ADAM_POW_ERR = 4 * 2.0 ** -24   # assumed absolute error of the device's b^t


def adam_bc64(t):
    """(bc1, bc2) = 1 - b^t in float64, b the device's float32 constants."""
    t = float(int(t))
    return (1.0 - float(np.float32(0.9)) ** t,
            1.0 - float(np.float32(0.999)) ** t)


def adam_lerp_oracle(p, g, m, v, tgt, t, lr, tau, scale=1.0, *, got):
    """One element-wise Adam step and target soft update, float64 arithmetic
    on float32 inputs, as k_adam_lerp / k_adam_lerp_clip / p_adam_lerp spell
    it:

        gs = scale * g                    (rounded once to float32)
        m' = b1 m + (1 - b1) gs           v' = b2 v + (1 - b2) gs^2
        p' = p - lr (m' / bc1) / (sqrt(v' / bc2) + eps),   bc_k = 1 - b_k^t
        tgt' = tgt + tau (p' - tgt)

    The constants are the device's: b1, b2, eps, lr, tau and scale rounded to
    float32, 1 - b formed in float32 (both differences are exact there).

    Each stage is teacher-forced on the device's own stored output of the
    stage before (`got`: dict with the device's "m", "v", "p"), so one stage's
    rounding never enters the next stage's comparison.  Returns
    {name: (expected, bound)} for m, v, p, tgt, float64, elementwise.

    Bounds (u = 2^-23; every float32 operation is taken to err by at most
    2^-24 relative, or 2^-150 absolute where its result is subnormal):
      m'   3 roundings (two products, one sum; an fma saves one):
           3u (|b1 m| + |(1-b1) gs|) + 2^-149
      v'   4 roundings ((1-b2) gs, that times gs, b2 v, the sum):
           4u (b2 v + (1-b2) gs^2) + 2^-149
      p'   u (|p_ref| + 6 |step|) + |step| (E1 + E2 / 2).  The step takes at
           most 8 roundings (1 - b1^t, m'/bc1, 1 - b2^t and v'/bc2 under the
           square root so halved, sqrt, + eps, lr *, the quotient), 7u/2, and
           the final subtraction u/2 of |p'|.  E_k = ADAM_POW_ERR / bc_k is
           the relative error bc_k inherits from the device's b_k^t; bc2
           stands under the square root, hence E2 / 2.
      tgt' p' - tgt, tau * that, and the sum (an fma saves one):
           u (|tgt_ref| + 2 tau |p' - tgt|)
    """
    f32, f64 = np.float32, np.float64
    b1, b2, eps = f32(0.9), f32(0.999), f32(1e-8)
    omb1, omb2 = f64(f32(1) - b1), f64(f32(1) - b2)
    lr, tau = f64(f32(lr)), f64(f32(tau))
    p, g, m, v, tgt = (np.asarray(x, f32) for x in (p, g, m, v, tgt))
    tiny = 2.0 ** -149
    gs = (f32(scale) * g).astype(f32).astype(f64)     # one float32 rounding
    m64, v64 = m.astype(f64), v.astype(f64)
    m_ref = f64(b1) * m64 + omb1 * gs
    m_bound = 3 * ADAM_U * (np.abs(f64(b1) * m64) + np.abs(omb1 * gs)) + tiny
    v_ref = f64(b2) * v64 + omb2 * gs * gs
    v_bound = 4 * ADAM_U * v_ref + tiny

    bc1, bc2 = adam_bc64(t)
    e1, e2 = ADAM_POW_ERR / bc1, ADAM_POW_ERR / bc2
    dm, dv = np.asarray(got["m"], f32).astype(f64), \
        np.asarray(got["v"], f32).astype(f64)
    step = lr * (dm / bc1) / (np.sqrt(dv / bc2) + f64(eps))
    p_ref = p.astype(f64) - step
    p_bound = (ADAM_U * (np.abs(p_ref) + 6 * np.abs(step))
               + np.abs(step) * (e1 + e2 / 2))

    dp, t64 = np.asarray(got["p"], f32).astype(f64), tgt.astype(f64)
    t_ref = t64 + tau * (dp - t64)
    t_bound = ADAM_U * (np.abs(t_ref) + 2 * tau * np.abs(dp - t64))
    return {"m": (m_ref, m_bound), "v": (v_ref, v_bound),
            "p": (p_ref, p_bound), "tgt": (t_ref, t_bound)}


# the edge classes of the Adam tests: (g, m, v, d) with tgt = p + d, except
# where d is a callable of p.  One block of these repeats through every slab.
def _rel(r):
    return lambda p: (p.astype(np.float64) * r).astype(np.float32) - p


ADAM_EDGES = [
    # name, g, m, v, d
    ("zero", 0.0, 0.0, 0.0, 0.5),
    ("g+tiny", 1e-18, 0.0, 0.0, -0.25),
    ("g-tiny", -1e-18, 0.0, 0.0, 0.25),
    ("big+", 1e3, 1e2, 1e6, 0.0),
    ("big-", -1e3, -1e2, 1e6, 0.0),
    ("big+-", 1e3, -1e2, 1e6, 0.125),
    ("cancel+", -9e-3, 1e-3, 1e-6, 0.0),
    ("cancel-", 9e-2, -1e-2, 1e-4, 0.0),
    ("eps+", 0.0, 1e-3, 1e-20, 0.0),
    ("eps-", 0.0, -1e-3, 1e-20, 0.0),
    ("tgt=p", None, None, None, 0.0),
    ("tgt=p+1", None, None, None, 1.0),
    ("tgt=p-1", None, None, None, -1.0),
    ("tgt=p(1+1e-7)", None, None, None, _rel(1 + 1e-7)),
    ("tgt=p(1-1e-7)", None, None, None, _rel(1 - 1e-7)),
    ("tgt=1e4", None, None, None, lambda p: np.float32(1e4) - p),
]
ADAM_PERIOD = 61     # prime: the block lands on every thread and stride slot


def adam_fill(n, seed, p=None, modest=False):
    """Five float32 slabs of n elements: a seeded normal bulk (p ~ 0.1 N, g ~
    1e-2 N, m ~ 1e-3 N, v ~ (1e-3 N)^2, tgt = p + 0.1 N: the targets are
    decoupled from the online net) and, at every index i with i % ADAM_PERIOD
    < len(ADAM_EDGES), edge class i % ADAM_PERIOD (None keeps the bulk value).
    `p` overrides the bulk parameters (a real net's slab).  modest: the
    eps-dominated classes carry m = +-1e-7, a step of about 10 * lr in place
    of 1e5 * lr, for slabs a forward pass still has to run on after the
    update.  Returns (dict of slabs, klass) with klass[i] the edge index or -1
    in the bulk."""
    f = np.float32
    rng = np.random.default_rng(seed)
    s = {"p": (0.1 * rng.standard_normal(n)).astype(f),
         "g": (1e-2 * rng.standard_normal(n)).astype(f),
         "m": (1e-3 * rng.standard_normal(n)).astype(f),
         "v": ((1e-3 * rng.standard_normal(n)) ** 2).astype(f)}
    if p is not None:
        s["p"] = np.asarray(p, f).copy()
    d = (0.1 * rng.standard_normal(n)).astype(f)
    idx = np.arange(n) % ADAM_PERIOD
    klass = np.where(idx < len(ADAM_EDGES), idx, -1)
    for k, (ename, g, m, v, dd) in enumerate(ADAM_EDGES):
        at = klass == k
        for name, val in (("g", g), ("m", m), ("v", v)):
            if val is not None:
                if modest and name == "m" and ename.startswith("eps"):
                    val = 1e-7 * np.sign(val)
                s[name][at] = f(val)
        d[at] = dd(s["p"][at]) if callable(dd) else f(dd)
    s["tgt"] = (s["p"] + d).astype(f)
    return s, klass
