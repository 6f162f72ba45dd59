"""HIP extension loader + the fused-engine wrapper.

The compiled extension (`_d4pg_hip.so`, built in-tree by setup.py /
__graft_entry__.build()) owns all GPU state: parameter slabs (weights stored
transposed [in][out]), Adam moments, target slabs, the on-HBM PER sum/min
trees and SoA replay store, device RNG and schedule counters.  Python only
packs/unpacks torch state_dicts into flat slabs and drives
step/capture/replay.

Policy: on a GPU machine the HIP path is mandatory — a missing or broken
extension raises ImportError loudly (no silent eager fallback; eager exists
for CPU tests only).
"""

from __future__ import annotations

import glob
import importlib.util
import os

import numpy as np
import torch

from ..config import check_gemm_precision

_EXT = None
_EXT_ERR: Exception | None = None


def _find_so():
    here = os.path.dirname(os.path.abspath(__file__))
    cands = sorted(glob.glob(os.path.join(here, "_d4pg_hip*.so")))
    return cands[0] if cands else None


def load_extension():
    """Import the in-tree compiled extension (no JIT — the .so must have
    been built by setup.py / __graft_entry__.build())."""
    global _EXT, _EXT_ERR
    if _EXT is not None:
        return _EXT
    so = _find_so()
    if so is None:
        _EXT_ERR = ImportError(
            "_d4pg_hip.so not found — build it with "
            "`python setup.py build_ext --inplace` (or __graft_entry__.build())")
        raise _EXT_ERR
    spec = importlib.util.spec_from_file_location("_d4pg_hip", so)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    _EXT = mod
    return mod


def extension_available() -> bool:
    try:
        load_extension()
        return True
    except Exception:
        return False


# ---------------------------------------------------------------------------
# slab packing: torch module (fc1/fc2/fc2_2/fc3) <-> flat engine slab
# ---------------------------------------------------------------------------

_LAYERS = ["fc1", "fc2", "fc2_2", "fc3"]


def pack_net(module: torch.nn.Module) -> torch.Tensor:
    """Flatten a 4-layer MLP into the engine slab layout:
    per layer, transposed weight [in][out] then bias [out]."""
    parts = []
    for name in _LAYERS:
        lin = getattr(module, name)
        parts.append(lin.weight.detach().t().contiguous().reshape(-1))
        parts.append(lin.bias.detach().reshape(-1))
    return torch.cat(parts).to(torch.float32).cpu()


def unpack_net(module: torch.nn.Module, flat: torch.Tensor) -> None:
    off = 0
    with torch.no_grad():
        for name in _LAYERS:
            lin = getattr(module, name)
            o, i = lin.weight.shape
            w = flat[off:off + i * o].reshape(i, o).t()
            off += i * o
            b = flat[off:off + o]
            off += o
            lin.weight.copy_(w)
            lin.bias.copy_(b)
    assert off == flat.numel(), "slab size mismatch on unpack"


# ---------------------------------------------------------------------------
# GPU replay adapter (host-side buffering -> batched device ingestion)
# ---------------------------------------------------------------------------

class GPUReplayAdapter:
    """Drop-in for the learner's replayBuffer when the replay lives on-HBM.
    add() buffers host-side; flush() ships one batched ingest (H2D + a
    single level-synced tree-insert kernel)."""

    def __init__(self, engine: "FusedEngine"):
        self.engine = engine
        self._pending = []
        self._batches = []

    def add(self, state, action, reward, next_state, done):
        self._pending.append((
            np.asarray(state, np.float32).ravel(),
            np.asarray(action, np.float32).ravel(),
            np.float32(reward),
            np.asarray(next_state, np.float32).ravel(),
            np.float32(done)))
        if len(self._pending) >= 32768:
            self.flush()

    def add_batch(self, states, actions, rewards, next_states, dones):
        """Array-form ingestion (the distributed learner's exchange path
        decodes whole SoA blocks — a per-transition python loop was the
        learner's bottleneck at high actor counts)."""
        self._batches.append((
            np.asarray(states, np.float32),
            np.asarray(actions, np.float32),
            np.asarray(rewards, np.float32).ravel(),
            np.asarray(next_states, np.float32),
            np.asarray(dones, np.float32).ravel()))

    def flush(self):
        parts = list(self._batches)
        self._batches.clear()
        if self._pending:
            parts.append((
                np.stack([p[0] for p in self._pending]),
                np.stack([p[1] for p in self._pending]),
                np.asarray([p[2] for p in self._pending], np.float32),
                np.stack([p[3] for p in self._pending]),
                np.asarray([p[4] for p in self._pending], np.float32)))
            self._pending.clear()
        for s, a, r, s2, d in parts:
            self.engine.ingest(torch.from_numpy(s), torch.from_numpy(a),
                               torch.from_numpy(r), torch.from_numpy(s2),
                               torch.from_numpy(d))

    def __len__(self):
        return (int(self.engine.counters()["size"]) + len(self._pending)
                + sum(len(b[2]) for b in self._batches))

    # -- exact resume (SURVEY §5 checkpoint row): snapshot/restore the
    # on-HBM SoA store + sum/min trees (zero-length on uniform replay) --
    def state_dict(self):
        self.flush()
        return dict(self.engine.ext.replay_state(self.engine.h))

    def load_state_dict(self, st):
        snap_per = st["sum_tree"].numel() > 0
        if snap_per != self.engine.prioritized:
            raise ValueError(
                "checkpoint replay mode (%s) does not match this engine's "
                "(%s) — there is no conversion between the two; build the "
                "agent with prioritized_replay=%r or pass load_replay=False"
                % ("prioritized" if snap_per else "uniform",
                   "prioritized" if self.engine.prioritized else "uniform",
                   snap_per))
        self._pending.clear()
        self.engine.ext.load_replay_state(
            self.engine.h, st["s"], st["a"], st["r"], st["s2"], st["d"],
            st["sum_tree"], st["min_tree"], int(st["size"]), int(st["pos"]),
            float(st["max_priority"]))


# ---------------------------------------------------------------------------
# the fused engine wrapper
# ---------------------------------------------------------------------------

class FusedEngine:
    """Owns one device-side D4PG learner (see ops/hip/engine.hip)."""

    def __init__(self, obs_dim, act_dim, hidden, n_atoms, batch, capacity,
                 v_min, v_max, gamma_n, tau, lr_actor, lr_critic,
                 per_alpha=0.6, per_beta0=0.4, per_beta_iters=100000,
                 per_eps=1e-6, seed=0, is_weighting=False,
                 prioritized=True, true_td_priorities=False,
                 gemm_precision="fp32", max_grad_norm=0.0,
                 dist="categorical", kappa=1.0):
        """prioritized=False: uniform replay (an integer philox draw per
        probe, IS weights exactly 1, no sum/min trees allocated or
        maintained).  true_td_priorities: the written-back priority is
        |E_m[z] - E_q[z]| + per_eps in place of the reference's <m, q>
        proxy.  gemm_precision="bf16": the GEMMs of the wide train step
        (batch > 512) round both operands to bf16 and accumulate in fp32;
        parameters, moments, activations and the replay stay fp32, and so do
        the rollout and evaluation forwards (ARCHITECTURE.md, "bf16 wide
        path").  The engine refuses it at batch <= 512.  max_grad_norm > 0:
        global-norm gradient clipping, the rule of
        torch.nn.utils.clip_grad_norm_ applied to the actor and to the
        critic separately, on all three train paths; Adam consumes the
        scaled gradient while g_actor / g_critic keep the raw one
        (ARCHITECTURE.md, "Gradient clipping").  0 is off; the engine
        refuses a negative or NaN threshold.  dist="quantile": the
        quantile-regression critic head on all three train paths — n_atoms
        quantiles at tau_i = (2i + 1) / (2 n_atoms), identity heads,
        quantile-Huber loss with threshold kappa > 0, priorities
        |mean T - mean theta| + per_eps whatever true_td_priorities says;
        v_min / v_max are unread (ARCHITECTURE.md, "Quantile critic").  The
        engine refuses an unknown dist and a kappa that is <= 0 or NaN; the
        categorical engine ignores kappa."""
        check_gemm_precision(gemm_precision)
        self.ext = load_extension()
        self.h = self.ext.create(
            obs_dim, act_dim, hidden, n_atoms, batch, capacity,
            float(v_min), float(v_max), float(gamma_n), float(tau),
            float(lr_actor), float(lr_critic), float(per_alpha),
            float(per_beta0), int(per_beta_iters), float(per_eps),
            int(seed), bool(is_weighting), bool(prioritized),
            bool(true_td_priorities), gemm_precision == "bf16",
            float(max_grad_norm), str(dist), float(kappa))
        self.dist = str(dist)
        self.kappa = float(kappa)
        self.batch = batch
        self.max_grad_norm = float(max_grad_norm)
        self.gemm_precision = gemm_precision
        self.prioritized = bool(prioritized)
        self._captured = 0
        self._persistent = bool(self.ext.info(self.h).get("persistent", False))

    def __del__(self):
        try:
            self.ext.destroy(self.h)
        except Exception:
            pass

    # -- params --
    SLABS = {"actor": 0, "actor_target": 1, "critic": 2, "critic_target": 3,
             "g_actor": 4, "g_critic": 5, "m_actor": 6, "v_actor": 7,
             "m_critic": 8, "v_critic": 9}

    # split-step phase masks (engine.hip enum): the learner-DP path runs
    # GRADS, all-reduces the grad slab over RCCL, then runs APPLY.
    PH_CRITIC_GRADS = 1
    PH_CRITIC_APPLY = 2
    PH_ACTOR_GRADS = 4
    PH_ACTOR_APPLY = 8
    PH_ALL = 15

    def load_from_modules(self, actor, actor_target, critic, critic_target):
        self.ext.load_slab(self.h, 0, pack_net(actor))
        self.ext.load_slab(self.h, 1, pack_net(actor_target))
        self.ext.load_slab(self.h, 2, pack_net(critic))
        self.ext.load_slab(self.h, 3, pack_net(critic_target))

    def store_to_modules(self, actor, actor_target, critic, critic_target):
        unpack_net(actor, self.ext.store_slab(self.h, 0))
        unpack_net(actor_target, self.ext.store_slab(self.h, 1))
        unpack_net(critic, self.ext.store_slab(self.h, 2))
        unpack_net(critic_target, self.ext.store_slab(self.h, 3))

    def load_slab(self, name, flat):
        self.ext.load_slab(self.h, self.SLABS[name], flat)

    def store_slab(self, name):
        return self.ext.store_slab(self.h, self.SLABS[name])

    # -- replay --
    def synth_fill(self, n, seed=1234):
        self.ext.synth_fill(self.h, int(n), int(seed))

    # device staging buffer rows per ingest call (engine.hip ing_cap)
    INGEST_CHUNK = 65536

    def ingest(self, s, a, r, s2, d):
        """Append transitions; chunks transparently at the engine's
        staging-buffer capacity (large actor pushes — e.g. GPU-rollout
        ranks at hundreds of envs — exceed one staging buffer)."""
        n = int(r.numel() if hasattr(r, "numel") else len(r))
        if n <= self.INGEST_CHUNK:
            self.ext.ingest(self.h, s, a, r, s2, d)
            return
        for lo in range(0, n, self.INGEST_CHUNK):
            hi = min(n, lo + self.INGEST_CHUNK)
            self.ext.ingest(self.h, s[lo:hi], a[lo:hi], r[lo:hi],
                            s2[lo:hi], d[lo:hi])

    def device_slab(self, name) -> torch.Tensor:
        """Zero-copy torch CUDA view of an engine slab — feed directly to
        torch.distributed collectives (RCCL).  Aliases engine memory."""
        return self.ext.device_tensor(self.h, self.SLABS[name])

    # -- stepping --
    def step(self, n=1):
        """Uncaptured (eager-launch) steps — used by parity tests."""
        self.ext.step(self.h, int(n))

    def step_part(self, mask):
        """Run only the PH_* phases of one train step (synchronizing), so
        the caller can all-reduce gradient slabs between GRADS and APPLY
        (learner data parallelism, SURVEY §2c collectives list)."""
        self.ext.step_part(self.h, int(mask))

    def train_steps(self, n=1, steps_per_graph=8):
        """Graph-replayed steps: captures once (steps_per_graph per replay),
        then replays; the remainder runs uncaptured.  On the persistent-
        megakernel path this is a single multi-step launch instead (no graph
        needed — the step loop lives inside the kernel)."""
        if self._persistent:
            self.ext.step(self.h, int(n))
            return
        if self._captured != steps_per_graph:
            self.ext.capture(self.h, steps_per_graph)
            self._captured = steps_per_graph
        full, rem = divmod(int(n), steps_per_graph)
        if full:
            self.ext.replay(self.h, full)
        if rem:
            self.ext.step(self.h, rem)

    def train_steps_async(self, n, steps_per_graph=8):
        if self._captured != steps_per_graph:
            self.ext.capture(self.h, steps_per_graph)
            self._captured = steps_per_graph
        assert n % steps_per_graph == 0
        self.ext.replay_async(self.h, n // steps_per_graph)

    def sync(self):
        self.ext.sync(self.h)

    # -- introspection / resume --
    def counters(self):
        return self.ext.counters(self.h)

    def grad_stats(self):
        """Gradient norms and clip scales of the last train step:
        norm_actor / norm_critic (float64, of the raw gradient slabs) and
        scale_actor / scale_critic (float32, what Adam multiplied by).
        All zero on an engine without clipping, which never computes them.
        One small device-to-host copy; call after the step has been
        synchronised."""
        return dict(self.ext.grad_stats(self.h))

    def set_schedule(self, steps_done, max_priority=1.0):
        """Restore schedule counters to 'steps_done completed' (resume).
        Counters live in device memory (read by the kernels each step), so
        no graph invalidation is needed here."""
        self.ext.set_schedule(self.h, int(steps_done), float(max_priority))

    def set_seed(self, seed):
        """Reseed the device philox stream.  The seed rides in captured
        kernel arguments, so this invalidates any captured hipGraph and
        forces a recapture on the next train_steps()."""
        self.ext.set_seed(self.h, int(seed))
        self._captured = 0

    def read(self, name):
        return self.ext.read_buffer(self.h, name)

    def actor_forward(self, x):
        return self.ext.actor_forward(self.h, x)

    # -- GPU-resident rollout (device Pendulum env + K11 noise + K15 fold,
    # transitions written straight into this engine's on-HBM replay;
    # see engine.hip "GPU-resident actor rollout") --
    def rollout_alloc(self, n_envs, n_steps, horizon=200, gamma=0.99,
                      noise="gaussian", eps=0.3, ou_theta=0.15,
                      ou_sigma=0.2, ou_mu=0.0, seed=0):
        kind = {"gaussian": 0, "ou": 1}[noise]
        self.ext.rollout_alloc(self.h, int(n_envs), int(n_steps),
                               int(horizon), float(gamma), kind, float(eps),
                               float(ou_theta), float(ou_sigma),
                               float(ou_mu), int(seed))

    def rollout_run(self, episodes=1, reset=True, use_graph=True):
        """Run whole episodes on-device (one hipGraph per episode when
        reset=True); returns (env_steps, transitions_emitted)."""
        self.ext.rollout_run(self.h, int(episodes), bool(reset),
                             bool(use_graph))
        info = self.ext.rollout_info(self.h)
        return (episodes * info["env_steps_per_episode"],
                episodes * info["emits_per_episode"])

    def rollout_set_state(self, th, thdot):
        self.ext.rollout_set_state(self.h, torch.as_tensor(th),
                                   torch.as_tensor(thdot))

    def rollout_info(self):
        return self.ext.rollout_info(self.h)

    # -- GPU-resident goal rollout (device GoalReach env + noise + n-step
    # fold + "future" HER relabel, rows written straight into this engine's
    # on-HBM replay; see ops/hip/engine_goal.hip) --
    def goal_rollout_alloc(self, n_envs, n_steps, horizon=50, gamma=0.99,
                           speed=0.1, tol=0.05, her_ratio=0.8,
                           noise="gaussian", eps=0.3, ou_theta=0.15,
                           ou_sigma=0.2, ou_mu=0.0, seed=0):
        kind = {"gaussian": 0, "ou": 1}[noise]
        self.ext.goal_rollout_alloc(
            self.h, int(n_envs), int(n_steps), int(horizon), float(gamma),
            float(speed), float(tol), float(her_ratio), kind, float(eps),
            float(ou_theta), float(ou_sigma), float(ou_mu), int(seed))

    def goal_rollout_run(self, episodes=1, reset=True, use_graph=True):
        """Run whole episodes on-device (one hipGraph per episode when
        reset=True); returns (env_steps, rows_emitted, successes) summed
        over the episodes, all three read back from device words —
        env_steps is the sum of the per-env episode lengths."""
        return tuple(self.ext.goal_rollout_run(
            self.h, int(episodes), bool(reset), bool(use_graph)))

    def goal_rollout_set_state(self, pos, goal):
        self.ext.goal_rollout_set_state(self.h, torch.as_tensor(pos),
                                        torch.as_tensor(goal))

    def goal_rollout_info(self):
        return self.ext.goal_rollout_info(self.h)

    def goal_rollout_episode(self):
        """The last episode as the device recorded it: ep_pos
        [horizon+1, M, D], ep_act [horizon, M, D], goal [M, D], len [M] and
        succ [M] (steps past an env's len are stale)."""
        return dict(self.ext.goal_rollout_episode(self.h))

    # -- GPU-resident synthetic-spec rollout, any (obs, act): device
    # SyntheticEnv dynamics + noise + n-step fold, rows written straight
    # into this engine's on-HBM replay; see ops/hip/engine_synth.hip --
    def synth_rollout_alloc(self, n_envs, n_steps, W, U, horizon=1000,
                            gamma=0.99, act_high=1.0, proc_sigma=0.01,
                            noise="gaussian", eps=0.3, ou_theta=0.15,
                            ou_sigma=0.2, ou_mu=0.0, seed=0):
        """W [obs, obs] and U [act, obs] are the env's mixing matrices
        (SyntheticEnv.W / .U, VectorSynthetic.W / .U)."""
        kind = {"gaussian": 0, "ou": 1}[noise]
        self.ext.synth_rollout_alloc(
            self.h, int(n_envs), int(n_steps), int(horizon), float(gamma),
            float(act_high), float(proc_sigma), kind, float(eps),
            float(ou_theta), float(ou_sigma), float(ou_mu), int(seed),
            torch.as_tensor(np.asarray(W, np.float32)),
            torch.as_tensor(np.asarray(U, np.float32)))

    def synth_rollout_run(self, episodes=1, reset=True, use_graph=True):
        """Run whole episodes on-device (one hipGraph per episode when
        reset=True); returns (env_steps, transitions_emitted)."""
        self.ext.synth_rollout_run(self.h, int(episodes), bool(reset),
                                   bool(use_graph))
        info = self.ext.synth_rollout_info(self.h)
        return (episodes * info["env_steps_per_episode"],
                episodes * info["emits_per_episode"])

    def synth_rollout_set_state(self, state):
        self.ext.synth_rollout_set_state(
            self.h, torch.as_tensor(np.asarray(state, np.float32)))

    def synth_rollout_info(self):
        return self.ext.synth_rollout_info(self.h)

    # -- overlapped collection (ops/hip/engine_stage.hip): the allocated
    # producer's episodes on a second stream while this engine trains; rows
    # reach the replay at the commit (ARCHITECTURE.md, "Overlapped
    # collection") --
    def collect_alloc(self, max_episodes):
        """Allocate the staging store for windows of up to `max_episodes`
        device episodes (call after a *_rollout_alloc; a new one frees it)."""
        self.ext.collect_alloc(self.h, int(max_episodes))

    def collect_begin(self, episodes=1, use_graph=True):
        """Open a collection window: snapshot the actor, enqueue `episodes`
        episodes on the rollout stream and return at once.  step /
        train_steps / step_part / evaluate / ingest and the read accessors
        stay legal until collect_commit(); the sync rollout calls, the
        rollout allocators, set_seed and the replay save/load refuse."""
        self.ext.collect_begin(self.h, int(episodes), bool(use_graph))

    def collect_commit(self):
        """Close the window: copy its rows into the live ring on the
        learner stream (after every step issued so far), wait, and return
        (env_steps, rows) of the window."""
        return tuple(self.ext.collect_commit(self.h))

    def collect_pending(self):
        return bool(self.ext.collect_pending(self.h))

    # -- device greedy evaluation (ops/hip/engine_eval.hip): noise-free
    # episodes of the allocated rollout producer's env, in a pool of their
    # own; nothing training reads is written --
    def eval_alloc(self, n_envs, horizon=None, seed=None, fixed_starts=False):
        """Allocate `n_envs` evaluation envs of the allocated rollout's kind
        (call after a *_rollout_alloc; a new one drops the evaluation).
        horizon None: the rollout's.  seed None: the rollout seed ^
        0x5EEDE7A1.  fixed_starts: every episode starts from the same states
        (and process noise), for common random numbers across checkpoints."""
        self.ext.eval_alloc(self.h, int(n_envs),
                            0 if horizon is None else int(horizon),
                            seed is not None,
                            0 if seed is None else int(seed),
                            bool(fixed_starts))

    def evaluate(self, episodes=1, use_graph=True):
        """Run `episodes` greedy episodes over the evaluation envs (one
        hipGraph launch each) and read the reduced result back in one copy."""
        episodes = int(episodes)
        if episodes < 1:
            raise ValueError("evaluate: episodes < 1")
        self.ext.eval_run(self.h, episodes, bool(use_graph))
        r = self.ext.eval_results(self.h)
        n = int(r["count"])
        return dict(mean_return=float(r["sum"]) / n,
                    min_return=float(r["min"]), max_return=float(r["max"]),
                    success_rate=int(r["successes"]) / n,
                    env_steps=int(r["env_steps"]), episodes=episodes)

    def eval_returns(self):
        """(ret float64, len int32, succ int32) per env of the last
        evaluation episode."""
        ret, ln, succ = self.ext.eval_arrays(self.h)
        return ret.numpy(), ln.numpy(), succ.numpy()

    # test hooks of the evaluation (tests/test_gpu_eval.py); not part of the
    # product surface
    def eval_results(self):
        """Test hook: the raw result words of the last evaluate() call."""
        return dict(self.ext.eval_results(self.h))

    def eval_set_state(self, x, y=None):
        """Test hook: start the next evaluation episode from the given env
        state — (th, thdot) for Pendulum, (pos, goal) for GoalReach, (state,)
        for the synthetic envs."""
        x = torch.as_tensor(np.asarray(x, np.float32))
        y = (torch.zeros(0) if y is None
             else torch.as_tensor(np.asarray(y, np.float32)))
        self.ext.eval_set_state(self.h, x, y)

    def eval_info(self):
        """Test hook: E, horizon, seed and fixed_starts as eval_alloc
        settled them."""
        return dict(self.ext.eval_info(self.h))

    def rollout_words(self):
        """Test hook: the eight per-episode device words of the allocated
        rollout."""
        return self.ext.rollout_words(self.h).numpy()

    def rollout_last_rows(self):
        """Host copy of the rows of the LAST rollout episode only, in write
        order, from its replay base and row count (replay_rows() returns
        every occupied slot).  After a collect_commit(): the committed
        block, from its live base."""
        base, count = self.ext.rollout_last(self.h)
        s, a, r, s2, d = self.ext.replay_slice(self.h, int(base), int(count))
        return (s.numpy(), a.numpy(), r.numpy().ravel(), s2.numpy(),
                d.numpy().ravel())

    def replay_rows(self):
        """Host copy of the occupied replay rows (s, a, r, s2, d) — used
        by GPU actor ranks to ship device-generated transitions to the
        learner, and by tests."""
        st = self.ext.replay_state(self.h)
        return (st["s"].numpy(), st["a"].numpy(),
                st["r"].numpy().ravel(), st["s2"].numpy(),
                st["d"].numpy().ravel())

    def info(self):
        return self.ext.info(self.h)


class FusedDDPGBridge:
    """Glue between the Python DDPG object and the device engine for the
    'hip' backend: replaces the replay with a GPUReplayAdapter, runs train
    steps on-device, and lazily syncs parameters back to the torch modules
    for acting/eval/checkpointing."""

    def __init__(self, ddpg):
        self.ddpg = ddpg
        self.engine = FusedEngine(
            obs_dim=ddpg.obs_dim, act_dim=ddpg.act_dim,
            hidden=ddpg.actor.hidden, n_atoms=ddpg.n_atoms,
            batch=ddpg.batch_size, capacity=ddpg.memory_size,
            v_min=ddpg.v_min, v_max=ddpg.v_max, gamma_n=ddpg.n_step_gamma,
            tau=ddpg.tau,
            lr_actor=ddpg.optimizer_actor.param_groups[0]["lr"],
            lr_critic=ddpg.optimizer_critic.param_groups[0]["lr"],
            is_weighting=ddpg.is_weighting,
            prioritized=ddpg.prioritized_replay,
            true_td_priorities=ddpg.true_td_priorities,
            gemm_precision=ddpg.gemm_precision,
            max_grad_norm=ddpg.max_grad_norm,
            dist=ddpg.dist_type, kappa=ddpg.kappa,
            seed=0 if ddpg.rng is None else int(ddpg.rng.integers(1 << 31)))
        self.engine.load_from_modules(ddpg.actor, ddpg.actor_target,
                                      ddpg.critic, ddpg.critic_target)
        # migrate any CPU replay contents, then swap in the GPU adapter
        adapter = GPUReplayAdapter(self.engine)
        old = getattr(ddpg, "replayBuffer", None)
        if old is not None and len(old) > 0:
            st = getattr(old, "_store", None) or getattr(old, "store", None)
            if st is not None and st.size > 0:
                n = st.size
                self.engine.ingest(
                    torch.from_numpy(st.states[:n]),
                    torch.from_numpy(st.actions[:n]),
                    torch.from_numpy(st.rewards[:n]),
                    torch.from_numpy(st.next_states[:n]),
                    torch.from_numpy(st.dones[:n]))
        ddpg.replayBuffer = adapter
        self._params_dirty = False

    def step(self, batch=None, n=1):
        self.ddpg.replayBuffer.flush()
        self.engine.train_steps(n)
        self._params_dirty = True
        self.ddpg.train_steps_done += n
        return float("nan"), float("nan")

    def sync_params_if_dirty(self):
        if self._params_dirty:
            self.engine.store_to_modules(
                self.ddpg.actor, self.ddpg.actor_target,
                self.ddpg.critic, self.ddpg.critic_target)
            self._params_dirty = False


def build_fused_engine(ddpg):
    if not torch.cuda.is_available():
        raise RuntimeError(
            "backend='hip' requires a GPU (use backend='eager' on CPU)")
    return FusedDDPGBridge(ddpg)
