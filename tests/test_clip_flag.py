"""--clip_grad_norm through the CLI, the config dataclass and the agent, and
the eager backend's clipped step against a hand-written clip of an unclipped
twin's gradients.  No GPU."""

import numpy as np
import pytest
import torch

from d4pg_amd.algo.d4pg import DDPG
from d4pg_amd.config import D4PGConfig, make_parser

O, A, H, B = 3, 1, 32, 16
DIST = {"type": "categorical", "v_min": -300.0, "v_max": 0.0, "n_atoms": 11}


def test_flag_default_is_off():
    args = make_parser().parse_args([])
    assert args.clip_grad_norm == 0.0
    assert D4PGConfig().clip_grad_norm == 0.0


def test_flag_parses_and_reaches_the_config():
    args = make_parser().parse_args(["--clip_grad_norm", "2.5"])
    assert args.clip_grad_norm == 2.5
    cfg = D4PGConfig.from_args(args)
    assert cfg.clip_grad_norm == 2.5
    assert "clip_grad_norm" not in cfg.extra


def test_train_main_passes_the_flag(monkeypatch):
    """train.main builds its agent with --clip_grad_norm."""
    import train

    class Built(Exception):
        pass

    def fake_ddpg(*a, **kw):
        raise Built(kw.get("max_grad_norm"))

    monkeypatch.setattr(train, "DDPG", fake_ddpg)
    for argv, want in ((["--clip_grad_norm", "0.5"], 0.5), ([], 0.0)):
        with pytest.raises(Built) as e:
            train.main(["--env", "Pendulum-v1", "--backend", "eager",
                        "--device", "cpu"] + argv)
        assert e.value.args[0] == want


@pytest.mark.parametrize("bad", [-1.0, float("nan")])
def test_negative_or_nan_threshold_is_refused(bad):
    with pytest.raises(ValueError, match="max_grad_norm"):
        DDPG(O, A, backend="eager", max_grad_norm=bad)


def _agent(**kw):
    return DDPG(O, A, memory_size=64, batch_size=B, prioritized_replay=False,
                critic_dist_info=DIST, hidden=H, backend="eager", seed=3,
                lr_actor=1e-3, lr_critic=1e-3, **kw)


def _batch():
    rng = np.random.default_rng(5)
    return (rng.standard_normal((B, O)).astype("f"),
            rng.uniform(-1, 1, (B, A)).astype("f"),
            rng.uniform(-30, 0, B).astype("f"),
            rng.standard_normal((B, O)).astype("f"),
            (rng.random(B) < 0.2).astype("f"), None, None)


def _grads(module):
    return [p.grad.detach().clone() for p in module.parameters()]


def _exp_avg(opt, module):
    return [opt.state[p]["exp_avg"] for p in module.parameters()]


def _norm(gs):
    return float(torch.sqrt(sum((g.double() ** 2).sum() for g in gs)))


def _critic_grads_at_init():
    """The critic's gradient on the fixed batch at the initial weights, read
    where the optimizer would consume it (the policy backward later adds to
    the critic's .grad); this twin's optimizers do not step."""
    probe, snap = _agent(), []
    probe.optimizer_critic.step = lambda: snap.extend(_grads(probe.critic))
    probe.optimizer_actor.step = lambda: None
    probe._train_step_eager(_batch())
    return snap


def test_eager_clip_matches_hand_clipped_gradients():
    """One train step on a fixed batch.  Adam's first exp_avg is
    (1 - beta1) * g, so it shows the gradient Adam consumed: it must be the
    unclipped twin's gradient times min(1, c / (norm + 1e-6)), per net.
    The critic's gradient is that of the common initial weights; the actor's
    is taken through the critic AFTER its (clipped) update, so the twin's
    critic is given the clipped agent's updated critic before its actor
    gradient is read."""
    plain = _agent()
    plain._train_step_eager(_batch())
    # critic gradient at the common initial weights, from an unclipped twin
    # whose optimizers do not step
    gc = _critic_grads_at_init()
    nc = _norm(gc)
    c = 0.5 * nc                            # the critic is clipped
    clipped = _agent(max_grad_norm=c)
    clipped._train_step_eager(_batch())
    sc = min(1.0, c / (nc + 1e-6))
    assert sc < 1.0
    for m, g in zip(_exp_avg(clipped.optimizer_critic, clipped.critic), gc):
        torch.testing.assert_close(m, 0.1 * (sc * g), rtol=1e-5, atol=1e-12)

    # actor gradient through the clipped agent's updated critic
    probe2 = _agent()
    probe2.critic.load_state_dict(clipped.critic.state_dict())
    s = torch.as_tensor(_batch()[0])
    z = probe2._z.reshape(-1, 1)
    loss = -(probe2.critic(s, probe2.actor(s)).matmul(z)).mean()
    probe2.actor.zero_grad()
    loss.backward()
    ga = _grads(probe2.actor)
    na = _norm(ga)
    sa = min(1.0, c / (na + 1e-6))
    for m, g in zip(_exp_avg(clipped.optimizer_actor, clipped.actor), ga):
        torch.testing.assert_close(m, 0.1 * (sa * g), rtol=1e-5, atol=1e-12)
    # and the clip changed something: the unclipped agent's moments differ
    m0 = _exp_avg(plain.optimizer_critic, plain.critic)[0]
    m1 = _exp_avg(clipped.optimizer_critic, clipped.critic)[0]
    assert not torch.allclose(m0, m1, rtol=1e-3, atol=0)


def test_threshold_zero_is_bitwise_the_agent_without_the_argument():
    a, b = _agent(), _agent(max_grad_norm=0.0)
    for _ in range(3):
        la = a._train_step_eager(_batch())
        lb = b._train_step_eager(_batch())
        assert la == lb
    for ma, mb in ((a.actor, b.actor), (a.critic, b.critic),
                   (a.actor_target, b.actor_target),
                   (a.critic_target, b.critic_target)):
        for pa, pb in zip(ma.parameters(), mb.parameters()):
            assert torch.equal(pa, pb)
    for oa, ob, mod_a, mod_b in ((a.optimizer_actor, b.optimizer_actor,
                                  a.actor, b.actor),
                                 (a.optimizer_critic, b.optimizer_critic,
                                  a.critic, b.critic)):
        for pa, pb in zip(mod_a.parameters(), mod_b.parameters()):
            assert torch.equal(oa.state[pa]["exp_avg"], ob.state[pb]["exp_avg"])
            assert torch.equal(oa.state[pa]["exp_avg_sq"],
                               ob.state[pb]["exp_avg_sq"])


def test_hogwild_path_clips_before_the_gradients_reach_the_global_model():
    """With a global model the local gradients are clipped before they are
    aliased into it, so the global optimizer consumes the clipped gradient."""
    gc = _critic_grads_at_init()
    c = 0.5 * _norm(gc)
    sc = min(1.0, c / (_norm(gc) + 1e-6))

    glob = _agent()
    local = _agent(max_grad_norm=c)
    oa = torch.optim.Adam(glob.actor.parameters(), lr=1e-3)
    oc = torch.optim.Adam(glob.critic.parameters(), lr=1e-3)
    local.assign_global_optimizer(oa, oc)
    local._train_step_eager(_batch(), glob)
    for p, g in zip(glob.critic.parameters(), gc):
        torch.testing.assert_close(oc.state[p]["exp_avg"], 0.1 * (sc * g),
                                   rtol=1e-5, atol=1e-12)


class _Recorder:
    def __init__(self):
        self.tags = []

    def add_scalar(self, tag, val, step):
        self.tags.append(tag)


def test_worker_scalars_need_the_flag_and_the_hip_backend():
    """grad_norm_scalars(): the two tags with the flag on the hip backend,
    nothing otherwise (an unclipped or eager run logs what it always did)."""
    from types import SimpleNamespace
    from d4pg_amd.parallel.worker import Worker

    class Eng:
        calls = 0

        def grad_stats(self):
            Eng.calls += 1
            return dict(norm_actor=1.5, norm_critic=2.5, scale_actor=1.0,
                        scale_critic=0.5)

    def worker(backend, clip):
        agent = SimpleNamespace(backend=backend,
                                engine=SimpleNamespace(engine=Eng()))
        args = SimpleNamespace(seed=0, clip_grad_norm=clip, vector_envs=0,
                               gpu_actors=-1, async_collect=0)
        return Worker("1", args, agent, env=None)

    assert worker("hip", 0.7).grad_norm_scalars() == [
        ("grad_norm_actor", 1.5), ("grad_norm_critic", 2.5)]
    calls = Eng.calls
    assert worker("hip", 0.0).grad_norm_scalars() == []
    assert worker("eager", 0.7).grad_norm_scalars() == []
    assert Eng.calls == calls          # no device read without the flag
