"""Shared kit of the GPU engine tests: builders, snapshots, the eager oracle.

One copy of what every GPU test file needs to set an engine up and to compare
two of them.  Bounds, tolerances, shape lists and buffer lists stay in the
test files, next to the comments that justify them; nothing here is cached.
The RNG call order of `modules` and `transitions` is part of the contract:
recorded figures (PARITY.md) rest on the exact inputs they produce.
"""

import copy

import numpy as np
import pytest
import torch

import _oracles as orc

PARAMS = ["actor", "actor_target", "critic", "critic_target"]
SLABS = PARAMS + ["g_actor", "g_critic", "m_actor", "v_actor", "m_critic",
                  "v_critic"]
INT_COUNTERS = ["beta_t", "adam_t_actor", "adam_t_critic", "rng_epoch",
                "size", "pos"]
LAYERS = ["fc1", "fc2", "fc2_2", "fc3"]


def pack(module, get=lambda p: p):
    """Per-parameter tensors (the parameter, its .grad, an Adam moment) in
    the engine slab layout: per layer, transposed weight then bias."""
    parts = []
    for n in LAYERS:
        lin = getattr(module, n)
        parts.append(get(lin.weight).t().contiguous().reshape(-1))
        parts.append(get(lin.bias).reshape(-1))
    return torch.cat(parts).detach().numpy()


def slabs_of(a, at, c, ct, opt_a, opt_c):
    """Parameter, target and Adam moment slabs of four nets and their two
    torch.optim.Adam optimizers."""
    out = {"actor": pack(a), "actor_target": pack(at), "critic": pack(c),
           "critic_target": pack(ct)}
    for tag, net, opt in (("actor", a, opt_a), ("critic", c, opt_c)):
        out["m_" + tag] = pack(net, lambda p: opt.state[p]["exp_avg"])
        out["v_" + tag] = pack(net, lambda p: opt.state[p]["exp_avg_sq"])
    return out


class Shape:
    def __init__(self, B, H, O, A, K, prioritized=True, precision="fp32",
                 head="categorical", v_min=-300.0, v_max=0.0, kappa=1.0):
        self.B, self.H, self.O, self.A, self.K = B, H, O, A, K
        self.prioritized, self.precision = prioritized, precision
        self.head, self.v_min, self.v_max, self.kappa = head, v_min, v_max, kappa
        self.path = ("persistent" if B <= 256 else
                     "rowblock" if B <= 512 else "wide")

    @property
    def dist(self):
        if self.head == "quantile":
            return {"type": "quantile", "n_atoms": self.K, "kappa": self.kappa}
        return {"type": "categorical", "v_min": self.v_min,
                "v_max": self.v_max, "n_atoms": self.K}

    def __repr__(self):
        return (f"B{self.B}-H{self.H}-O{self.O}-A{self.A}-K{self.K}"
                + ("" if self.prioritized else "-uniform")
                + ("" if self.precision == "fp32" else "-" + self.precision))


def modules(shape, seed):
    """(actor, actor_target, critic, critic_target): one torch.manual_seed,
    the actor, then the critic; the targets are deep copies."""
    from d4pg_amd.models import actor, critic
    torch.manual_seed(seed)
    a = actor(shape.O, shape.A, hidden=shape.H)
    c = critic(shape.O, shape.A, shape.dist, hidden=shape.H)
    return a, copy.deepcopy(a), c, copy.deepcopy(c)


def draw_rows(rng, O, A, n, r_range=(-30, 0), p_done=0.05):
    """Five draws from `rng`, in the order s, a, r, s2, d."""
    return (rng.standard_normal((n, O)).astype("f"),
            rng.uniform(-1, 1, (n, A)).astype("f"),
            rng.uniform(*r_range, n).astype("f"),
            rng.standard_normal((n, O)).astype("f"),
            (rng.random(n) < p_done).astype("f"))


def transitions(shape, n, seed, r_range=(-30, 0), p_done=0.05):
    return draw_rows(np.random.default_rng(seed), shape.O, shape.A, n,
                     r_range, p_done)


def engine(shape, mods=None, rows=None, *, capacity, seed=13,
           gamma_n=0.99 ** 5, tau=1e-3, lr=1e-4, **engine_kw):
    """The FusedEngine of `shape` with the suite's common hyper-parameters.
    Any constructor argument can be given in engine_kw (one that is None is
    not forwarded); mods are loaded and rows ingested when given."""
    from d4pg_amd.ops import FusedEngine
    kw = dict(obs_dim=shape.O, act_dim=shape.A, hidden=shape.H,
              n_atoms=shape.K, batch=shape.B, capacity=capacity,
              v_min=shape.v_min, v_max=shape.v_max, gamma_n=gamma_n, tau=tau,
              lr_actor=lr, lr_critic=lr, seed=seed)
    if not shape.prioritized:
        kw["prioritized"] = False
    if shape.precision != "fp32":
        kw["gemm_precision"] = shape.precision
    if shape.head != "categorical":
        kw.update(dist=shape.head, kappa=shape.kappa)
    kw.update({k: v for k, v in engine_kw.items() if v is not None})
    eng = FusedEngine(**kw)
    if mods is not None:
        eng.load_from_modules(*mods)
    if rows is not None:
        eng.ingest(*[torch.from_numpy(x) for x in rows])
    return eng


def snapshot(eng, buffers, slabs=SLABS, counters=INT_COUNTERS):
    """(arrays and integer counters by name, the full counters dict)."""
    st = {"slab:" + n: eng.store_slab(n).numpy() for n in slabs}
    st.update({n: eng.read(n).numpy() for n in buffers})
    cnt = eng.counters()
    st.update({"cnt:" + n: cnt[n] for n in counters})
    return st, cnt


def assert_bitwise(x, y, what, loss_rel=1e-5):
    sx, cx = x
    sy, cy = y
    assert sx.keys() == sy.keys(), f"{what}: {sorted(sx.keys() ^ sy.keys())}"
    for k in sx:
        assert np.array_equal(sx[k], sy[k]), f"{what}: {k} differs"
    # the loss scalars accumulate through cross-workgroup fp32 atomics,
    # whose order is not fixed: approximately equal only
    for k in ("loss_critic", "loss_actor"):
        assert cx[k] == pytest.approx(cy[k], rel=loss_rel), f"{what}: {k}"


def assert_bs_is_gathered(eng, what):
    """read('bs') resolves the parity buffer the last step used."""
    idx = eng.read("bidx").numpy()
    assert np.array_equal(eng.read("bs").numpy(), eng.replay_rows()[0][idx]), \
        f"{what}: bs is not the gathered batch"


# ---------------------------------------------------------------------------
# eager torch replica of one train step on a given batch
# ---------------------------------------------------------------------------

class CategoricalHead:
    """Categorical projection, cross-entropy, <q, z> policy loss."""

    def __init__(self, v_min, v_max, gamma_n, n_atoms):
        self.v_min, self.v_max, self.gamma_n = v_min, v_max, gamma_n
        self.z = torch.linspace(v_min, v_max, n_atoms).reshape(-1, 1)

    def target(self, p_t, r, d):
        from d4pg_amd.algo.projection import categorical_projection
        return categorical_projection(p_t, r, d, self.v_min, self.v_max,
                                      self.gamma_n)

    def critic_loss(self, q, T):
        return -(T * torch.log(q + 1e-10)).sum(1)

    def policy_loss(self, pq):
        return -(pq.matmul(self.z)).mean()


class QuantileHead:
    """Quantile targets, quantile-Huber loss, mean-of-quantiles policy
    loss."""

    def __init__(self, gamma_n, kappa):
        self.gamma_n, self.kappa = gamma_n, kappa

    def target(self, p_t, r, d):
        from d4pg_amd.algo.quantile import quantile_targets
        return quantile_targets(p_t, r, d, self.gamma_n)

    def critic_loss(self, q, T):
        from d4pg_amd.algo.quantile import quantile_huber_loss
        return quantile_huber_loss(q, T, self.kappa)

    def policy_loss(self, pq):
        return -pq.mean(dim=1).mean()


class Eager:
    """critic Adam, policy gradient through the UPDATED critic, actor Adam,
    both soft updates (test_post_step_params_parity's order)."""

    def __init__(self, mods, lr, tau, *, head):
        self.a, self.at, self.c, self.ct = [copy.deepcopy(m) for m in mods]
        self.opt_c = torch.optim.Adam(self.c.parameters(), lr=lr)
        self.opt_a = torch.optim.Adam(self.a.parameters(), lr=lr)
        self.tau, self.head = tau, head

    def step(self, s, act, r, s2, d, w=None):
        s, act, r, s2, d = [torch.from_numpy(x) for x in (s, act, r, s2, d)]
        with torch.no_grad():
            self.a2 = self.at(s2)
            self.p_t = self.ct(s2, self.a2)
            self.T = self.head.target(self.p_t, r, d)
        self.q = self.c(s, act)
        rows = self.head.critic_loss(self.q, self.T)
        loss_c = (rows if w is None else torch.from_numpy(w) * rows).mean()
        self.c.zero_grad()
        loss_c.backward()
        # (the policy loss below also backpropagates into the critic)
        self.g_critic = pack(self.c, lambda p: p.grad.clone())
        self.opt_c.step()
        pl = self.head.policy_loss(self.c(s, self.a(s)))
        self.a.zero_grad()
        pl.backward()
        self.opt_a.step()
        with torch.no_grad():
            for tp, sp in zip(self.at.parameters(), self.a.parameters()):
                tp.lerp_(sp, self.tau)
            for tp, sp in zip(self.ct.parameters(), self.c.parameters()):
                tp.lerp_(sp, self.tau)

    def grads(self):
        """Gradients of the LAST step, in the engine's slab layout."""
        return {"g_actor": pack(self.a, lambda p: p.grad),
                "g_critic": self.g_critic}

    def slabs(self):
        return slabs_of(self.a, self.at, self.c, self.ct, self.opt_a,
                        self.opt_c)


# ---------------------------------------------------------------------------
# an injected, non-uniform prioritized replay
# ---------------------------------------------------------------------------

def per_replay(shape, size, seed=0):
    """Rows by name, and leaf priorities log-uniform over six decades."""
    rng = np.random.default_rng(seed)
    rp = dict(zip(("s", "a", "r", "s2", "d"),
                  draw_rows(rng, shape.O, shape.A, size)))
    rp["leaves"] = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), size))
    return rp


def inject_replay(eng, rp, max_priority=1.0):
    """Load rows and the trees built from rp['leaves'];
    (sum_tree, min_tree, tree_cap)."""
    cap = eng.info()["tree_cap"]
    size = len(rp["r"])
    st, mt = orc.build_trees(rp["leaves"], cap)
    eng.ext.load_replay_state(
        eng.h, *[torch.from_numpy(rp[k]) for k in ("s", "a", "r", "s2", "d")],
        torch.from_numpy(st), torch.from_numpy(mt), size, size,
        max_priority)
    return st, mt, cap


# ---------------------------------------------------------------------------
# a hip-backend agent for the checkpoint tests
# ---------------------------------------------------------------------------

CATEGORICAL = {"type": "categorical", "v_min": -300.0, "v_max": 0.0,
               "n_atoms": 51}


def agent(dist=CATEGORICAL, *, memory_size, batch_size=64, prioritized=True,
          seed=0, **kw):
    from d4pg_amd.algo.d4pg import DDPG
    return DDPG(3, 1, memory_size=memory_size, batch_size=batch_size,
                critic_dist_info=dist, n_steps=5, gamma=0.99,
                prioritized_replay=prioritized, device="cuda", backend="hip",
                seed=seed, **kw)


def fill_agent(agent, n, seed=7, reward=lambda rng: -rng.random(),
               done=lambda rng: 0.0):
    """n rows through replayBuffer.add, drawn per row in the order s, a,
    reward(rng), s2, done(rng)."""
    rng = np.random.default_rng(seed)
    for _ in range(n):
        agent.replayBuffer.add(rng.standard_normal(3).astype("f"),
                               rng.uniform(-1, 1, 1).astype("f"),
                               reward(rng),
                               rng.standard_normal(3).astype("f"), done(rng))


def flat_params(agent):
    from d4pg_amd.ops import pack_net
    agent.engine.sync_params_if_dirty()
    return torch.cat([pack_net(agent.actor), pack_net(agent.critic),
                      pack_net(agent.actor_target),
                      pack_net(agent.critic_target)]).numpy()


# ---------------------------------------------------------------------------
# the rollout producers' engine
# ---------------------------------------------------------------------------

def producer_nets(o, a, dist, *, hidden, actor_seed, critic_seed,
                  head_gain=None):
    """(actor, critic).  critic_seed None: the critic is drawn from the
    actor's RNG stream, continued; otherwise torch is re-seeded for it.
    head_gain scales the actor's 3e-3 head init, so that actions spread over
    (-1, 1) instead of sitting at 0."""
    from d4pg_amd.models import actor, critic
    torch.manual_seed(actor_seed)
    net = actor(o, a, hidden=hidden)
    if head_gain is not None:
        with torch.no_grad():
            net.fc3.weight.mul_(head_gain)
    if critic_seed is not None:
        torch.manual_seed(critic_seed)
    return net, critic(o, a, dist, hidden=hidden)


def producer_engine(o, a, *, hidden, n_atoms, capacity, batch=64, seed=0,
                    v_min, v_max, gamma_n, lr, prioritized=True, actor_seed,
                    critic_seed, head_gain=None, actor=None):
    """(engine, actor): the actor is loaded as online and target net, and so
    is the critic.  `actor`: a net to load in place of the seeded one."""
    dist = {"type": "categorical", "v_min": v_min, "v_max": v_max,
            "n_atoms": n_atoms}
    net, c = producer_nets(o, a, dist, hidden=hidden, actor_seed=actor_seed,
                           critic_seed=critic_seed, head_gain=head_gain)
    net = actor or net
    shape = Shape(batch, hidden, o, a, n_atoms, prioritized=prioritized,
                  v_min=v_min, v_max=v_max)
    return engine(shape, (net, net, c, c), capacity=capacity, seed=seed,
                  gamma_n=gamma_n, lr=lr), net
