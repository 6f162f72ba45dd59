"""Global-norm gradient clipping on the fused engine (max_grad_norm), all three
train paths: persistent (B <= 256), row-block (256 < B <= 512 and every split
step) and wide (B > 512).

Per net: norm = sqrt(sum g^2) over the whole gradient slab in double, scale =
float32(min(1, c / (norm + 1e-6))), Adam consumes scale * g and the slab keeps
the raw gradient.  Adam's first parameter step is invariant to a constant
gradient scale (m / sqrt(v) is +-1), so the checks read the m and v slabs, and
compare parameters only after several steps.

The thresholds come from a same-seed engine WITHOUT clipping run for one step
(_base, computed once per shape and never modified): with Na, Nc the float64
norms of its gradient slabs, "both" = 0.5 * min(Na, Nc) clips both nets and
"one" = sqrt(Na * Nc) clips exactly the net with the larger norm.
"""

import functools
import math

import numpy as np
import pytest

import _engine_kit as kit

pytestmark = pytest.mark.gpu

GAMMA_N = 0.99 ** 5
TAU, LR = 0.001, 1e-4
CAP, N = 4096, 1024
CHUNK = 4096                     # GN_CHUNK of ops/hip/engine_rowmath.hip
NETS = ("actor", "critic")


class Shape(kit.Shape):
    """The kit's shape with its inputs (seed B) and its unclipped first step
    computed once and shared."""

    @functools.lru_cache(maxsize=None)
    def modules(self):
        return kit.modules(self, self.B)

    @functools.lru_cache(maxsize=None)
    def transitions(self):
        return kit.transitions(self, N, self.B)

    def engine(self, max_grad_norm=None):
        """max_grad_norm None: an engine built without the argument."""
        eng = kit.engine(self, self.modules(), self.transitions(),
                         capacity=CAP, max_grad_norm=max_grad_norm)
        assert eng._persistent == (self.path == "persistent")
        return eng

    @functools.lru_cache(maxsize=None)
    def base(self):
        """One step of the unclipped engine: its gradient slabs, their
        float64 norms and the two thresholds."""
        eng = self.engine()
        eng.step(1)
        g = {n: eng.store_slab("g_" + n).numpy() for n in NETS}
        for v in g.values():
            v.setflags(write=False)
        na, nc = (float(np.sqrt(np.sum(g[n].astype(np.float64) ** 2)))
                  for n in NETS)
        return dict(g=g, Na=na, Nc=nc, both=0.5 * min(na, nc),
                    one=math.sqrt(na * nc), stats=eng.grad_stats(),
                    parts={n: eng.read("gn_part_" + n).numpy() for n in NETS})

    def threshold(self, mode):
        b = self.base()
        if mode == "one":
            # the geometric mean separates the nets only if the norms differ
            r = max(b["Na"], b["Nc"]) / min(b["Na"], b["Nc"])
            assert r > 1.05, f"{self!r}: norms {b['Na']}, {b['Nc']} too close"
        return b[mode]


P8 = Shape(8, 64, 3, 1, 11)          # one column tile; ~9k-element slabs:
#                                      two full chunks and a ragged one
P50 = Shape(50, 128, 17, 6, 51)      # partial last row group, act > 1
RB = Shape(300, 128, 3, 1, 51)       # row-block
WIDE = Shape(520, 100, 3, 1, 51)     # ragged tiles, empty split-K tails
WIDE_BF16 = Shape(520, 100, 3, 1, 51, precision="bf16")
P8_UNIFORM = Shape(8, 64, 3, 1, 11, prioritized=False)
ALL = [P8, P50, RB, WIDE, WIDE_BF16, P8_UNIFORM]
PER_PATH = [P50, RB, WIDE]           # one shape per path


def _slabs(eng):
    return kit.snapshot(eng, [], counters=[])[0]


def _same(x, y, what):
    assert x.keys() == y.keys()
    for k in x:
        assert np.array_equal(x[k], y[k]), f"{what}: {k} differs"


def _f64_norm(g):
    return float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))


def _chunk_sums(g):
    sq = g.astype(np.float64) ** 2
    return np.array([sq[i:i + CHUNK].sum() for i in range(0, sq.size, CHUNK)])


# ---------------------------------------------------------------------------
# 1. norm, scale, partials
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["both", "one"])
@pytest.mark.parametrize("shape", ALL, ids=repr)
def test_norm_scale_and_partials(shape, mode):
    """Norms against numpy float64 at 1e-10 (both sides sum < 1e6 exact double
    squares: ordering error <= n * 2^-53), the float32 scale bitwise from the
    device's own double norm, the per-chunk partials at 1e-12 (the ragged
    last chunk included)."""
    c = shape.threshold(mode)
    eng = shape.engine(max_grad_norm=c)
    eng.step(1)
    st = eng.grad_stats()
    clipped = []
    for n in NETS:
        g = eng.store_slab("g_" + n).numpy()
        norm, scale = st["norm_" + n], st["scale_" + n]
        want = _f64_norm(g)
        parts, wparts = eng.read("gn_part_" + n).numpy(), _chunk_sums(g)
        print(f"{shape!r} {mode} {n}: norm {norm!r} numpy {want!r} rel "
              f"{abs(norm - want) / want:.2e} scale {scale!r} chunks "
              f"{parts.size} (last {g.size - (parts.size - 1) * CHUNK}) max "
              f"rel {np.abs(parts / wparts - 1).max():.2e}")
        assert abs(norm - want) <= 1e-10 * want
        assert np.float32(scale) == np.float32(min(1.0, c / (norm + 1e-6)))
        assert parts.shape == wparts.shape
        assert parts.size == -(-g.size // CHUNK)
        np.testing.assert_allclose(parts, wparts, rtol=1e-12, atol=0)
        clipped.append(scale < 1.0)
        if not clipped[-1]:
            assert scale == 1.0
    assert clipped == ([True, True] if mode == "both" else
                       [shape.base()["Na"] > shape.base()["Nc"],
                        shape.base()["Nc"] > shape.base()["Na"]])


# ---------------------------------------------------------------------------
# 2. the moments follow the fp32 recurrence on scale * g
# ---------------------------------------------------------------------------

def _recur(m, v, gs):
    b1, b2, one = np.float32(0.9), np.float32(0.999), np.float32(1)
    return b1 * m + (one - b1) * gs, b2 * v + (one - b2) * gs * gs


@pytest.mark.parametrize("mode", ["both", "one"])
@pytest.mark.parametrize("shape", ALL, ids=repr)
def test_moments_follow_the_scaled_gradient(shape, mode):
    """Three step(1) calls; after each, m and v must be the fp32 Adam
    recurrence on float32(scale) * g, scale from grad_stats(), within 1e-6 of
    the slab's largest entry (test_gpu_multistep's form for moments).  After
    the first step the UNSCALED recurrence must miss that bound on a clipped
    net and meet it on the unclipped one ("one")."""
    c = shape.threshold(mode)
    eng = shape.engine(max_grad_norm=c)
    m = {n: np.zeros_like(shape.base()["g"][n]) for n in NETS}
    v = {n: np.zeros_like(shape.base()["g"][n]) for n in NETS}
    for step in range(3):
        eng.step(1)
        st = eng.grad_stats()
        for n in NETS:
            g = eng.store_slab("g_" + n).numpy()
            scale = np.float32(st["scale_" + n])
            got_m = eng.store_slab("m_" + n).numpy()
            got_v = eng.store_slab("v_" + n).numpy()
            raw_m, raw_v = _recur(m[n], v[n], g)
            m[n], v[n] = _recur(m[n], v[n], scale * g)
            em = np.abs(got_m - m[n]).max() / np.abs(m[n]).max()
            ev = np.abs(got_v - v[n]).max() / np.abs(v[n]).max()
            rm = np.abs(got_m - raw_m).max() / np.abs(m[n]).max()
            rv = np.abs(got_v - raw_v).max() / np.abs(v[n]).max()
            print(f"{shape!r} {mode} step {step + 1} {n}: scale {scale!r} "
                  f"m err {em:.2e} v err {ev:.2e}; unscaled m {rm:.2e} "
                  f"v {rv:.2e}")
            assert em <= 1e-6 and ev <= 1e-6, (n, step)
            if step == 0:
                if scale < 1.0:
                    assert rm > 1e-6 and rv > 1e-6, \
                        f"{n}: Adam consumed the unscaled gradient"
                else:
                    assert rm <= 1e-6 and rv <= 1e-6
            # carry the device's own moments: errors do not compound
            m[n], v[n] = got_m, got_v


# ---------------------------------------------------------------------------
# 3. the gradient slabs stay raw
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ALL, ids=repr)
def test_gradient_slabs_stay_unscaled(shape):
    """Same weights, same batch, same forward and backward: the gradient
    slabs of a clipped first step are bitwise the unclipped twin's.  The
    critic's slab is compared with the critic clipped ("both" and "one").
    The actor's gradient is taken through the critic AFTER its update, and a
    clipped critic update is the twin's only up to Adam's eps (m / (sqrt(v) +
    1e-8) is not exactly scale-free), so the actor's slab is compared when the
    critic's scale is exactly 1.0 and the actor is the clipped net; where the
    critic has the larger norm no threshold does that, and the actor's slab is
    pinned raw by test_moments_follow_the_scaled_gradient alone (a slab scaled
    in place would make m follow scale^2 * g)."""
    b = shape.base()
    eng = shape.engine(max_grad_norm=shape.threshold("both"))
    eng.step(1)
    assert eng.grad_stats()["scale_critic"] < 1.0
    assert np.array_equal(eng.store_slab("g_critic").numpy(), b["g"]["critic"])
    eng = shape.engine(max_grad_norm=shape.threshold("one"))
    eng.step(1)
    st = eng.grad_stats()
    assert np.array_equal(eng.store_slab("g_critic").numpy(), b["g"]["critic"])
    print(f"{shape!r}: Na {b['Na']:.4g} Nc {b['Nc']:.4g} scales {st}")
    if st["scale_critic"] == 1.0:
        assert st["scale_actor"] < 1.0
        assert np.array_equal(eng.store_slab("g_actor").numpy(),
                              b["g"]["actor"])


# ---------------------------------------------------------------------------
# 4. the paths agree
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [P8, P50], ids=repr)
def test_persistent_and_rowblock_reductions_agree_bitwise(shape):
    """The persistent step against the row-block path's four step_part
    launches (the hook of tests/test_gpu_handoff.py), same weights and batch.
    The two paths' dW kernels round differently (test_gpu_handoff bounds
    their slabs at 1e-6, not bitwise), so the row-block engine is handed the
    persistent engine's gradient slab between GRADS and APPLY, as a
    data-parallel all-reduce would: norm, scale and partials of the two
    reductions over the same slab must then be bitwise equal."""
    c = shape.threshold("both")
    e1, e2 = shape.engine(max_grad_norm=c), shape.engine(max_grad_norm=c)
    e1.step(1)
    e2.step_part(e2.PH_CRITIC_GRADS)
    e2.load_slab("g_critic", e1.store_slab("g_critic"))
    e2.step_part(e2.PH_CRITIC_APPLY)
    e2.step_part(e2.PH_ACTOR_GRADS)
    e2.load_slab("g_actor", e1.store_slab("g_actor"))
    e2.step_part(e2.PH_ACTOR_APPLY)
    assert np.array_equal(e1.read("bidx").numpy(), e2.read("bidx").numpy())
    s1, s2 = e1.grad_stats(), e2.grad_stats()
    print(shape, s1, s2)
    assert s1 == s2
    for n in NETS:
        assert np.array_equal(e1.read("gn_part_" + n).numpy(),
                              e2.read("gn_part_" + n).numpy()), n


# ---------------------------------------------------------------------------
# 5. launch forms
# ---------------------------------------------------------------------------

def _full(eng):
    return _slabs(eng), eng.grad_stats()


def _same_full(x, y, what):
    _same(x[0], y[0], what)
    assert x[1] == y[1], f"{what}: grad_stats {x[1]} != {y[1]}"


@pytest.mark.parametrize("shape", [P8, P50, P8_UNIFORM], ids=repr)
def test_multistep_persistent_launch_equals_single_steps(shape):
    c = shape.threshold("both")
    x, y, z = (shape.engine(max_grad_norm=c) for _ in range(3))
    x.step(4)
    for _ in range(4):
        y.step(1)
    z.step(1)
    z.step(3)
    ref = _full(y)
    assert ref[1]["scale_critic"] < 1.0 or ref[1]["scale_actor"] < 1.0
    _same_full(_full(x), ref, "step(4) vs 4 x step(1)")
    _same_full(_full(z), ref, "step(1)+step(3) vs 4 x step(1)")
    assert y.counters()["adam_t_actor"] == 4


@pytest.mark.parametrize("shape", [RB, WIDE, WIDE_BF16], ids=repr)
def test_graph_replay_split_step_and_twin_equal_uncaptured(shape):
    c = shape.threshold("both")
    x, y, w = (shape.engine(max_grad_norm=c) for _ in range(3))
    x.step(4)
    ref = _full(x)
    y.train_steps(4, steps_per_graph=2)      # two replays of a 2-step graph
    assert y._captured == 2
    _same_full(_full(y), ref, "graph replay vs uncaptured")
    for _ in range(4):                       # the DPEngine order
        for mask in (w.PH_CRITIC_GRADS, w.PH_CRITIC_APPLY, w.PH_ACTOR_GRADS,
                     w.PH_ACTOR_APPLY):
            w.step_part(mask)
    _same_full(_full(w), ref, "split step vs full step")


@pytest.mark.parametrize("shape", ALL, ids=repr)
def test_same_seed_engines_are_equal(shape):
    c = shape.threshold("one")
    x, y = shape.engine(max_grad_norm=c), shape.engine(max_grad_norm=c)
    x.step(2)
    y.step(2)
    _same_full(_full(x), _full(y), "same-seed twins")


# ---------------------------------------------------------------------------
# 6. a threshold that never binds
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ALL, ids=repr)
def test_threshold_that_never_binds_changes_nothing(shape):
    """max_grad_norm=1e30: scales exactly 1.0, and after three steps all ten
    slabs are bitwise those of an engine built without the argument — the
    extra multiply and the extra barriers disturb nothing else."""
    x, y = shape.engine(max_grad_norm=1e30), shape.engine()
    for _ in range(3):
        x.step(1)
        st = x.grad_stats()
        assert st["scale_actor"] == 1.0 and st["scale_critic"] == 1.0
        assert st["norm_actor"] > 0 and st["norm_critic"] > 0
    y.step(3)
    _same(_slabs(x), _slabs(y), "1e30 vs no argument")
    assert x.info()["max_grad_norm"] == 1e30
    assert y.info()["max_grad_norm"] == 0.0


# ---------------------------------------------------------------------------
# 7. against the eager backend
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", PER_PATH, ids=repr)
def test_three_steps_match_the_eager_backend(shape):
    """DDPG(backend="eager", max_grad_norm=c) on the batches the engine drew.
    Parameters and targets at test_gpu_multistep's 6e-5, m and v at 1e-4 of
    the slab's largest entry."""
    from d4pg_amd.algo.d4pg import DDPG
    c = shape.threshold("both")
    eng = shape.engine(max_grad_norm=c)
    ag = DDPG(shape.O, shape.A, memory_size=8, batch_size=shape.B,
              lr_critic=LR, lr_actor=LR, gamma=GAMMA_N, tau=TAU,
              prioritized_replay=False, critic_dist_info=shape.dist,
              n_steps=1, backend="eager", hidden=shape.H, max_grad_norm=c)
    a, at, cr, ct = shape.modules()
    ag.actor.load_state_dict(a.state_dict())
    ag.actor_target.load_state_dict(at.state_dict())
    ag.critic.load_state_dict(cr.state_dict())
    ag.critic_target.load_state_dict(ct.state_dict())
    tr = shape.transitions()
    for _ in range(3):
        eng.step(1)
        idx = eng.read("bidx").numpy()
        ag._train_step_eager(tuple(t[idx] for t in tr) + (None, None))
    st = eng.grad_stats()
    assert st["scale_actor"] < 1.0 or st["scale_critic"] < 1.0
    want = kit.slabs_of(ag.actor, ag.actor_target, ag.critic,
                        ag.critic_target, ag.optimizer_actor,
                        ag.optimizer_critic)
    got = {n: eng.store_slab(n).numpy() for n in want}
    for n in want:
        print(f"{shape!r} {n}: max abs err {np.abs(got[n] - want[n]).max():.3g}"
              f" (max |ref| {np.abs(want[n]).max():.3g})")
    for n in want:
        np.testing.assert_allclose(got[n], want[n], atol=6e-5, err_msg=n)
    for n in ("m_actor", "m_critic", "v_actor", "v_critic"):
        assert np.abs(got[n] - want[n]).max() <= 1e-4 * np.abs(want[n]).max(), n


# ---------------------------------------------------------------------------
# 8. refusals and reporting
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [-1.0, float("nan")])
def test_engine_refuses_negative_or_nan_threshold(bad):
    with pytest.raises(RuntimeError, match="max_grad_norm"):
        P8.engine(max_grad_norm=bad)


@pytest.mark.parametrize("shape", PER_PATH, ids=repr)
def test_unclipped_engine_reports_zeros_and_computes_nothing(shape):
    """Without clipping the statistics block and the partials are never
    written: the reduction kernels and phases did not run."""
    b = shape.base()
    assert b["stats"] == dict(norm_actor=0.0, norm_critic=0.0,
                              scale_actor=0.0, scale_critic=0.0)
    for n in NETS:
        assert not b["parts"][n].any()


class _Recorder:
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, val, step):
        self.rows.append((tag, float(val)))


def _worker(tmp_path, extra=()):
    from d4pg_amd.algo.d4pg import DDPG
    from d4pg_amd.config import (configure_env_params, critic_dist_info,
                                 make_parser)
    from d4pg_amd.envs import make, obs_act_dims
    from d4pg_amd.parallel.worker import Worker
    args = make_parser().parse_args(
        ["--env", "Pendulum-v1", "--vector_envs", "64", "--max_steps", "20",
         "--n_steps", "3", "--warmup", "64", "--episodes_per_cycle", "64",
         "--train_steps_per_cycle", "4", "--eval_trials", "16", "--rmsize",
         "20000", "--bsize", "64", "--n_eps", "1", "--cycles_per_epoch", "1",
         "--debug", "0", "--seed", "0", *extra])
    configure_env_params(args)
    env = make(args.env, seed=0)
    env._max_episode_steps = args.max_steps
    obs_dim, act_dim = obs_act_dims(env, her=bool(args.her))
    agent = DDPG(obs_dim, act_dim, env=env, memory_size=args.rmsize,
                 batch_size=args.bsize, gamma=args.gamma, tau=args.tau,
                 prioritized_replay=True,
                 critic_dist_info=critic_dist_info(args),
                 n_steps=args.n_steps, device="cuda", backend="hip", seed=0,
                 max_grad_norm=args.clip_grad_norm)
    rec = _Recorder()
    w = Worker("t", args, agent, env, writer=rec, run_dir=str(tmp_path))
    w.work(max_cycles=1)
    return rec, agent


TODAY_TAGS = ["avg_test_reward", "success_rate", "grad_steps_per_sec",
              "env_steps_per_sec"]


def test_worker_logs_the_norms_only_with_the_flag(tmp_path):
    rec, agent = _worker(tmp_path)
    assert [t for t, _ in rec.rows] == TODAY_TAGS
    rec, agent = _worker(tmp_path, ("--clip_grad_norm", "0.01"))
    assert [t for t, _ in rec.rows] == TODAY_TAGS + ["grad_norm_actor",
                                                      "grad_norm_critic"]
    st = agent.engine.engine.grad_stats()
    assert dict(rec.rows)["grad_norm_actor"] == st["norm_actor"] > 0
    assert dict(rec.rows)["grad_norm_critic"] == st["norm_critic"] > 0
