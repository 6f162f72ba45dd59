"""--async_collect: the flag, the Worker's cycle order over a stub agent and
engine that record their calls, the episode rounding and the refusal when no
device collect path exists.  No GPU."""

import pytest

from d4pg_amd.config import D4PGConfig, make_parser
from d4pg_amd.parallel.worker import Worker

M, HOR, N = 64, 8, 3
ROWS = M * (HOR - N + 1)


class StubEngine:
    def __init__(self, log):
        self.log = log
        self.open = False

    def rollout_alloc(self, n_envs, n_steps, **kw):
        self.log.append(("rollout_alloc", n_envs))

    def rollout_run(self, episodes=1, **kw):
        assert not self.open
        self.log.append(("rollout_run", episodes))
        return episodes * M * HOR, episodes * ROWS

    def eval_alloc(self, n_envs, **kw):
        self.log.append(("eval_alloc", n_envs))

    def collect_alloc(self, max_episodes):
        self.log.append(("collect_alloc", max_episodes))
        self.max_episodes = max_episodes

    def collect_begin(self, episodes=1, use_graph=True):
        assert not self.open and episodes <= self.max_episodes
        self.open, self.episodes = True, episodes
        self.log.append(("collect_begin", episodes))

    def collect_commit(self):
        assert self.open
        self.open = False
        self.log.append(("collect_commit",))
        return self.episodes * M * HOR, self.episodes * ROWS

    def evaluate(self, episodes=1):
        assert not self.open
        self.log.append(("evaluate",))
        return dict(mean_return=-1.0, success_rate=0.0)


class StubBridge:
    def __init__(self, log):
        self.log = log
        self.engine = StubEngine(log)

    def step(self, batch=None, n=1):
        self.log.append(("train", n))


class StubReplay:
    def flush(self):
        pass


class StubAgent:
    def __init__(self, backend="hip"):
        self.backend = backend
        self.log = []
        self.engine = StubBridge(self.log)
        self.replayBuffer = StubReplay()
        self.memory_size = 100000
        self.train_steps_done = 0

    def ensure_engine(self):
        return self.engine

    def train(self, global_model=None):
        self.log.append(("train", 1))

    def save(self, run_dir):
        pass


class StubEnv:
    _max_episode_steps = HOR


def _args(*extra):
    return make_parser().parse_args(
        ["--env", "Pendulum-v1", "--vector_envs", str(M), "--n_steps",
         str(N), "--warmup", "64", "--episodes_per_cycle", "64",
         "--train_steps_per_cycle", "8", "--eval_trials", "16", "--n_eps",
         "1", "--cycles_per_epoch", "5", "--debug", "0", *extra])


def _run(args, cycles=2):
    agent = StubAgent()
    w = Worker("t", args, agent, StubEnv(), run_dir="")
    w.work(max_cycles=cycles)
    # one entry per train cycle (agent.train() + the engine's n - 1 steps)
    log = []
    for e in agent.log:
        if e[0] == "train" and log and log[-1][0] == "train":
            log[-1] = ("train", log[-1][1] + e[1])
        else:
            log.append(e)
    return w, log


def test_flag_parses_and_defaults_to_zero():
    assert _args().async_collect == 0
    assert _args("--async_collect", "1").async_collect == 1
    assert D4PGConfig().async_collect == 0
    assert D4PGConfig.from_args(_args("--async_collect", "1")) \
        .async_collect == 1
    with pytest.raises(SystemExit):
        _args("--async_collect", "2")


def test_async_cycle_order():
    w, log = _run(_args("--async_collect", "1"))
    cycle = [("collect_begin", 1), ("train", 8), ("collect_commit",),
             ("evaluate",)]
    assert log == [("rollout_alloc", M), ("eval_alloc", 16),
                   ("collect_alloc", 1),
                   ("rollout_run", 1)] + cycle + cycle     # serial warmup
    assert w.device_rows == 3 * ROWS
    assert w.env_meter.count == 3 * M * HOR


def test_episode_count_rounds_up():
    w, log = _run(_args("--async_collect", "1", "--episodes_per_cycle", "65",
                        "--warmup", "129"), cycles=1)
    assert ("collect_alloc", 2) in log and ("collect_begin", 2) in log
    assert ("rollout_run", 3) in log
    assert w.device_rows == 5 * ROWS


def test_serial_sequence_is_unchanged():
    for args in (_args(), _args("--async_collect", "0")):
        w, log = _run(args)
        cycle = [("rollout_run", 1), ("train", 8), ("evaluate",)]
        assert log == [("rollout_alloc", M), ("eval_alloc", 16),
                       ("rollout_run", 1)] + cycle + cycle
        assert w.device_rows == 3 * ROWS


@pytest.mark.parametrize("backend,extra", [
    ("eager", ()), ("hip", ("--vector_envs", "0")),
    ("hip", ("--gpu_actors", "0")), ("hip", ("--env", "NoSuchEnv-v0"))])
def test_refused_without_a_device_kind(backend, extra):
    args = _args("--async_collect", "1", *extra)
    with pytest.raises(ValueError) as e:
        Worker("t", args, StubAgent(backend), StubEnv(), run_dir="")
    for flag in ("--async_collect", "--backend", "--vector_envs",
                 "--gpu_actors"):
        assert flag in str(e.value)
    # the same flags without --async_collect construct as before
    args.async_collect = 0
    assert Worker("t", args, StubAgent(backend), StubEnv(),
                  run_dir="").device_kind() is None
