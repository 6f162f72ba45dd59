"""Worker: the per-process actor+learner loop, and the evaluator.

Schedule parity with the reference's ``Worker.work`` and
``global_model_eval`` (/root/reference/main.py:188-368, 103-134):

  per epoch: ``cycles_per_epoch`` cycles of
    { collect ``episodes_per_cycle`` episodes -> ``train_steps_per_cycle``
      gradient steps -> ``eval_trials`` greedy rollouts -> scalars
      ``avg_test_reward``/``success_rate`` -> actor.pth/critic.pth save }

with a warmup fill of ``warmup`` episodes before training
(main.py:200-243).  In multithread mode each Worker runs in its own process
against a shared-memory global model (parallel/hogwild.py); the evaluator
copies global weights every 10 s and rolls one greedy episode, maintaining
the 0.95/0.05 EWMA return (main.py:103-134).
"""

from __future__ import annotations

import os
import time

import numpy as np

from ..her import add_experience, rollout_episode
from ..utils.logging import Meter, SummaryWriter


class Worker:
    def __init__(self, name, args, agent, env, writer: SummaryWriter | None = None,
                 run_dir: str | None = None):
        self.name = str(name)
        self.args = args
        self.agent = agent
        self.env = env
        self.run_dir = run_dir or "."
        self.writer = writer
        self.grad_meter = Meter()
        self.env_meter = Meter()
        self.rng = np.random.default_rng(
            None if args.seed is None else args.seed + hash(self.name) % 1000)
        self._device_run = None     # the allocated producer's run method
        self.device_rows = 0        # replay rows the device episodes wrote
        self._device_kind = self._find_device_kind()
        # --async_collect 1: collection windows overlap the train cycle
        self._async = bool(int(getattr(args, "async_collect", 0)))
        if self._async and self._device_kind is None:
            raise ValueError(
                "--async_collect 1 overlaps DEVICE collection with training: "
                "it needs --backend hip, --vector_envs M > 0, --gpu_actors "
                "!= 0 and an env a device rollout models (Pendulum, "
                "GoalReach with --her 1, a synthetic env); got backend %r, "
                "--vector_envs %d, --gpu_actors %d, --env %r, --her %d"
                % (getattr(agent, "backend", "eager"),
                   int(getattr(args, "vector_envs", 0)),
                   int(getattr(args, "gpu_actors", -1)),
                   getattr(args, "env", None), int(getattr(args, "her", 0))))

    # -- the closed on-GPU cycle --
    # With backend 'hip', --vector_envs M > 0, --gpu_actors != 0 and an env
    # one of the device rollouts models (Pendulum; GoalReach with --her 1; an
    # env that unwraps to SyntheticEnv — the tests DistributedD4PG applies),
    # collection and evaluation run as device episodes on the learner's OWN
    # engine: rows go straight into the replay the fused step samples, the
    # policy is the p_actor slab the step updates (no parameter copy, no host
    # rows) and env.step is never called.  Episode counts round up to whole
    # batches of M envs.
    #
    # With --async_collect 1 the warmup stays serial and each cycle becomes
    # collect_begin(ceil(episodes_per_cycle / M)) -> train_cycle ->
    # collect_commit -> evaluate: the episodes run on the engine's rollout
    # stream with a snapshot of the actor while the learner trains, and
    # their rows enter the replay at the commit.  Rows collected with the
    # policy of cycle k are therefore sampled from cycle k+1 on (an actor
    # one window behind the learner, as across the distributed ranks).
    eval_fixed_starts = False   # common random numbers across evaluations

    def _find_device_kind(self):
        a = self.args
        if getattr(self.agent, "backend", "eager") != "hip":
            return None
        if int(getattr(a, "vector_envs", 0)) <= 0 \
                or int(getattr(a, "gpu_actors", -1)) == 0:
            return None
        from .vec_eval import env_kind
        return env_kind(a, self.env)

    def device_kind(self):
        """'pendulum' / 'goal' / 'synth' when this Worker takes the device
        path, else None (decided once, at construction)."""
        return self._device_kind

    def device_engine(self):
        """The learner's engine with this env's rollout producer and the
        evaluation allocated on it (built on first use)."""
        if self._device_run is not None:
            return self.agent.engine.engine
        from .vec_eval import alloc_producer, producer_rows
        a, kind = self.args, self._device_kind
        m = int(a.vector_envs)
        horizon = int(self.env._max_episode_steps)
        need = producer_rows(kind, m, horizon, a.n_steps)
        cap = int(getattr(self.agent, "memory_size", a.rmsize))
        if cap < need:
            raise ValueError(
                "--rmsize %d is below the %d rows one device episode of "
                "--vector_envs %d envs can write (M*(max_steps-n_steps+1)%s): "
                "two rows of one episode would share a replay slot; raise "
                "--rmsize or lower --vector_envs"
                % (cap, need, m,
                   " + M*max_steps hindsight rows" if kind == "goal" else ""))
        eng = self.agent.ensure_engine().engine
        seed = (0 if a.seed is None else int(a.seed)) + 37
        self._device_run = alloc_producer(eng, kind, a, self.env, m, seed)
        eng.eval_alloc(int(a.eval_trials), horizon=horizon,
                       fixed_starts=self.eval_fixed_starts)
        if self._async:
            eng.collect_alloc(self._window_episodes())
        return eng

    def _window_episodes(self) -> int:
        """Device episodes of one collection window: episodes_per_cycle
        rounded up to whole batches of M envs."""
        return -(-int(self.args.episodes_per_cycle)
                 // int(self.args.vector_envs))

    def collect_begin(self) -> None:
        """Open the cycle's collection window (returns at once)."""
        eng = self.device_engine()
        self.agent.replayBuffer.flush()
        eng.collect_begin(self._window_episodes())

    def collect_commit(self) -> None:
        """Close the window: its rows enter the replay after the cycle's
        train steps."""
        out = self.device_engine().collect_commit()
        self.env_meter.add(int(out[0]))
        self.device_rows += int(out[1])

    def _device_collect(self, episodes: int) -> None:
        if episodes <= 0:
            return
        self.device_engine()
        self.agent.replayBuffer.flush()
        m = int(self.args.vector_envs)
        out = self._device_run(-(-int(episodes) // m))
        self.env_meter.add(int(out[0]))
        self.device_rows += int(out[1])

    # -- warmup fill (reference main.py:200-243) --
    def warmup(self) -> None:
        if self._device_kind is not None:
            return self._device_collect(self.args.warmup)
        for _ in range(self.args.warmup):
            ep, _, _ = rollout_episode(self.agent, self.env, noise=True)
            self.env_meter.add(len(ep))
            add_experience(self.agent.replayBuffer, self.env, ep,
                           her=bool(self.args.her), n_steps=self.args.n_steps,
                           gamma=self.args.gamma, rng=self.rng)

    def collect_cycle(self) -> None:
        if self._device_kind is not None:
            return self._device_collect(self.args.episodes_per_cycle)
        for _ in range(self.args.episodes_per_cycle):
            ep, _, _ = rollout_episode(self.agent, self.env, noise=True)
            self.env_meter.add(len(ep))
            add_experience(self.agent.replayBuffer, self.env, ep,
                           her=bool(self.args.her), n_steps=self.args.n_steps,
                           gamma=self.args.gamma, rng=self.rng)

    def train_cycle(self, global_model=None, global_count=None) -> None:
        n = self.args.train_steps_per_cycle
        if global_model is None and self.agent.backend == "hip":
            # fused multi-step: one engine launch for the whole cycle
            self.agent.train()              # builds the bridge on first use
            if n > 1:
                self.agent.engine.step(n=n - 1)
            self.grad_meter.add(n)
            if global_count is not None:
                global_count += n
            return
        for _ in range(n):
            self.agent.train(global_model)
            self.grad_meter.add()
            if global_count is not None:
                global_count += 1     # HogWild-tolerated non-atomic increment

    def grad_norm_scalars(self):
        """With --clip_grad_norm > 0 on the hip backend: the gradient norms
        of the cycle's last train step, as (tag, value) pairs (one small
        device-to-host copy; the cycle's train steps have been synchronised).
        Empty otherwise, so an unclipped run logs what it always logged."""
        if float(getattr(self.args, "clip_grad_norm", 0.0)) <= 0.0 \
                or getattr(self.agent, "backend", "eager") != "hip" \
                or self.agent.engine is None:
            return []
        st = self.agent.engine.engine.grad_stats()
        return [("grad_norm_actor", float(st["norm_actor"])),
                ("grad_norm_critic", float(st["norm_critic"]))]

    def evaluate(self):
        if self._device_kind is not None:
            # eval_trials greedy device envs on the slab the step updates:
            # no sync_params_if_dirty()
            r = self.device_engine().evaluate(1)
            return float(r["mean_return"]), float(r["success_rate"])
        returns, successes = [], []
        for _ in range(self.args.eval_trials):
            _, R, s = rollout_episode(self.agent, self.env, noise=False)
            returns.append(R)
            successes.append(float(s))
        return float(np.mean(returns)), float(np.mean(successes))

    def work(self, global_model=None, global_count=None,
             max_cycles: int | None = None) -> None:
        """The main loop.  ``global_model``/``global_count`` engage
        HogWild-parity shared-memory training (main.py:245-307);
        ``max_cycles`` bounds the run (tests/bench)."""
        if global_model is not None:
            self.agent.sync_local_global(global_model)
            self.agent.hard_update()
        self.warmup()
        cycle_idx = 0
        for epoch in range(self.args.n_eps):
            for _ in range(self.args.cycles_per_epoch):
                if self._async:
                    self.collect_begin()
                    self.train_cycle(global_model, global_count)
                    self.collect_commit()
                else:
                    self.collect_cycle()
                    self.train_cycle(global_model, global_count)
                avg_r, succ = self.evaluate()
                step = (global_count.item() if global_count is not None
                        else self.agent.train_steps_done)
                if self.writer is not None:
                    self.writer.add_scalar("avg_test_reward", avg_r, step)
                    self.writer.add_scalar("success_rate", succ, step)
                    self.writer.add_scalar("grad_steps_per_sec",
                                           self.grad_meter.rate(), step)
                    self.writer.add_scalar("env_steps_per_sec",
                                           self.env_meter.rate(), step)
                    for tag, val in self.grad_norm_scalars():
                        self.writer.add_scalar(tag, val, step)
                if self.args.debug:
                    print(f"[worker {self.name}] epoch {epoch} step {step} "
                          f"avg_test_reward {avg_r:.2f} success {succ:.2f}",
                          flush=True)
                if self.run_dir:
                    os.makedirs(self.run_dir, exist_ok=True)
                    self.agent.save(self.run_dir)
                cycle_idx += 1
                if max_cycles is not None and cycle_idx >= max_cycles:
                    return


def global_model_eval(global_model, global_count, args, env_factory,
                      stop_at: float = 1e6, period: float = 10.0,
                      max_iters: int | None = None):
    """Evaluator process body (reference main.py:103-134): copy global
    weights, one greedy rollout, EWMA return, repeat every ``period`` s."""
    from ..algo.d4pg import DDPG
    from ..config import critic_dist_info

    env = env_factory()
    from ..envs import obs_act_dims
    obs_dim, act_dim = obs_act_dims(env, her=bool(args.her))
    agent = DDPG(obs_dim, act_dim, env=env, memory_size=1000,
                 batch_size=args.bsize, gamma=args.gamma, tau=args.tau,
                 prioritized_replay=False,
                 critic_dist_info=critic_dist_info(args),
                 n_steps=args.n_steps, seed=args.seed)
    ewma = None
    iters = 0
    while float(global_count.item()) < stop_at:
        agent.actor.load_state_dict(global_model.actor.state_dict())
        agent.critic.load_state_dict(global_model.critic.state_dict())
        _, R, _ = rollout_episode(agent, env, noise=False, max_steps=500)
        ewma = R if ewma is None else 0.95 * ewma + 0.05 * R
        print(f"[eval] step {int(global_count.item())} return {R:.2f} "
              f"ewma {ewma:.2f}", flush=True)
        iters += 1
        if max_iters is not None and iters >= max_iters:
            return ewma
        time.sleep(period)
    return ewma
