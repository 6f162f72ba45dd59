"""The quantile-regression critic head on the CPU: the pure loss function
against a float64 double loop, the identity-head critic, the eager DDPG train
step, checkpoints and the CLI flags."""

import copy

import numpy as np
import pytest
import torch

from d4pg_amd.algo.d4pg import DDPG
from d4pg_amd.algo.quantile import (quantile_huber_loss, quantile_targets,
                                    quantile_taus)
from d4pg_amd.config import critic_dist_info, make_parser
from d4pg_amd.models import critic

KAPPA = 1.0
GAMMA_N = 0.99 ** 3


def oracle_rows(theta, target, kappa):
    """float64 double loop over (i, j): row loss l, d l / d theta and the
    branch counts (|u| < kappa, |u| > kappa, u < 0, u == 0)."""
    theta = np.asarray(theta, np.float64)
    target = np.asarray(target, np.float64)
    B, K = theta.shape
    loss = np.zeros(B)
    grad = np.zeros((B, K))
    counts = dict(small=0, large=0, neg=0, zero=0)
    for b in range(B):
        for i in range(K):
            tau = (2 * i + 1) / (2.0 * K)
            for j in range(K):
                u = target[b, j] - theta[b, i]
                w = abs(tau - (1.0 if u < 0 else 0.0))
                if abs(u) <= kappa:
                    h = 0.5 * u * u
                else:
                    h = kappa * (abs(u) - 0.5 * kappa)
                loss[b] += w * h / kappa / K
                grad[b, i] += -w * min(max(u, -kappa), kappa) / kappa / K
                counts["small"] += abs(u) < kappa
                counts["large"] += abs(u) > kappa
                counts["neg"] += u < 0
                counts["zero"] += u == 0
    return loss, grad, counts


def branchy_batch(B, K, seed):
    """Online quantiles, target quantiles, rewards over about [-3, 3], a few
    done rows, and row 0 built so that some T_j == theta_i exactly."""
    rng = np.random.default_rng(seed)
    theta = rng.uniform(-2, 2, (B, K)).astype(np.float32)
    theta_t = rng.uniform(-2, 2, (B, K)).astype(np.float32)
    r = rng.uniform(-3, 3, B).astype(np.float32)
    d = (rng.random(B) < 0.25).astype(np.float32)
    d[0] = 1.0                      # T_0j = r_0 for every j ...
    theta[0, 0] = r[0]              # ... and theta_00 equals it: u == 0
    if B > 1:
        d[1] = 0.0
    return theta, theta_t, r, d


@pytest.mark.parametrize("K", [1, 11, 51, 64])
def test_quantile_huber_loss_matches_float64_loop(K):
    B = 6
    theta, theta_t, r, d = branchy_batch(B, K, seed=K)
    T = quantile_targets(torch.from_numpy(theta_t), torch.from_numpy(r),
                         torch.from_numpy(d), GAMMA_N)
    th = torch.from_numpy(theta).requires_grad_(True)
    loss = quantile_huber_loss(th, T, KAPPA)
    assert loss.shape == (B,)
    loss.sum().backward()
    want_l, want_g, counts = oracle_rows(theta, T.numpy(), KAPPA)
    # the inputs reach every branch (K = 1 has a single pair per row)
    assert counts["zero"] >= 1, counts
    if K > 1:
        for k in ("small", "large", "neg"):
            assert counts[k] >= K, counts
    # fp32 pairwise sums over K^2 terms of size <= ~6: a few ulp of the sum
    np.testing.assert_allclose(loss.detach().numpy(), want_l,
                               rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(th.grad.numpy(), want_g, rtol=2e-5, atol=1e-6)
    # targets are constants
    assert not T.requires_grad


def test_quantile_taus_and_kappa_check():
    np.testing.assert_allclose(quantile_taus(4).numpy(),
                               [0.125, 0.375, 0.625, 0.875])
    th = torch.zeros(2, 3)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            quantile_huber_loss(th, th, bad)


def test_loss_scales_with_kappa():
    """H / kappa: for |u| <= kappa halving kappa doubles the loss."""
    th = torch.zeros(1, 1)
    T = torch.full((1, 1), 0.25)
    l1 = float(quantile_huber_loss(th, T, 1.0))
    l2 = float(quantile_huber_loss(th, T, 0.5))
    assert l1 == pytest.approx(0.5 * 0.5 * 0.25 ** 2)
    assert l2 == pytest.approx(2 * l1)
    # and beyond kappa it is linear: kappa * (|u| - kappa / 2) / kappa
    l3 = float(quantile_huber_loss(th, T, 0.125))
    assert l3 == pytest.approx(0.5 * (0.25 - 0.0625))


# ---------------------------------------------------------------------------
# the critic module
# ---------------------------------------------------------------------------

QDIST = {"type": "quantile", "n_atoms": 11, "kappa": 1.0}


def test_quantile_critic_is_identity_head():
    torch.manual_seed(0)
    c = critic(5, 2, QDIST, hidden=32)
    s, a = torch.randn(7, 5), torch.rand(7, 2)
    out = c(s, a)
    assert out.shape == (7, 11)
    assert torch.equal(out, c.logits(s, a))
    # same keys and shapes as the categorical critic
    cat = critic(5, 2, {"type": "categorical", "v_min": -1.0, "v_max": 1.0,
                        "n_atoms": 11}, hidden=32)
    assert {k: v.shape for k, v in c.state_dict().items()} == \
        {k: v.shape for k, v in cat.state_dict().items()}
    cat.load_state_dict(c.state_dict())
    assert torch.allclose(cat(s, a), torch.softmax(out, dim=-1))


def test_quantile_critic_refuses_log():
    c = critic(5, 2, QDIST, hidden=32)
    with pytest.raises(ValueError):
        c(torch.randn(2, 5), torch.rand(2, 2), log=True)


def test_mixture_still_rejected():
    with pytest.raises(NotImplementedError):
        critic(3, 1, {"type": "mixture_of_gaussian", "n_atoms": 51})
    with pytest.raises(NotImplementedError):
        DDPG(3, 1, critic_dist_info={"type": "mixture_of_gaussian",
                                     "n_atoms": 51}, hidden=16)


# ---------------------------------------------------------------------------
# the eager learner
# ---------------------------------------------------------------------------

def _agent(dist, seed=3, **kw):
    agent = DDPG(5, 2, memory_size=512, batch_size=16, n_steps=3,
                 critic_dist_info=dist, hidden=32, backend="eager", seed=seed,
                 **kw)
    rng = np.random.default_rng(seed)
    for _ in range(128):
        agent.replayBuffer.add(rng.standard_normal(5).astype("f"),
                               rng.uniform(-1, 1, 2).astype("f"),
                               float(rng.uniform(-3, 3)),
                               rng.standard_normal(5).astype("f"),
                               float(rng.random() < 0.1))
    return agent


def test_eager_quantile_step_trains():
    agent = _agent(dict(QDIST))
    before = copy.deepcopy(agent.critic.state_dict())
    for _ in range(3):
        lc, la = agent.train()
        assert np.isfinite(lc) and np.isfinite(la)
    assert any(not torch.equal(before[k], v)
               for k, v in agent.critic.state_dict().items())
    # priorities written back: |mean T - mean theta| + eps >= eps, finite
    leaves = np.asarray(agent.replayBuffer.state_dict()["leaves"])
    assert np.isfinite(leaves).all()
    assert (leaves >= agent.prioritized_replay_eps ** 0.6 * (1 - 1e-12)).all()


def test_eager_quantile_step_matches_formulas():
    """One eager step's critic gradient is (1/B) sum_b dl_b/dtheta pushed
    through the critic: check it at the head against the float64 oracle."""
    agent = _agent(dict(QDIST), prioritized_replay=False)
    batch = agent.sample(16)
    s, a, r, s2, d = [torch.as_tensor(np.asarray(x, np.float32))
                      for x in batch[:5]]
    with torch.no_grad():
        T = quantile_targets(
            agent.critic_target(s2, agent.actor_target(s2)), r, d,
            agent.n_step_gamma)
    theta = agent.critic(s, a).detach().requires_grad_(True)
    quantile_huber_loss(theta, T, agent.kappa).mean().backward()
    _, want_g, _ = oracle_rows(theta.detach().numpy(), T.numpy(), agent.kappa)
    np.testing.assert_allclose(theta.grad.numpy(), want_g / 16, rtol=2e-5,
                               atol=1e-7)
    lc, la = agent._train_step_eager(batch)
    want_l, _, _ = oracle_rows(theta.detach().numpy(), T.numpy(), agent.kappa)
    assert lc == pytest.approx(want_l.mean(), rel=1e-5)


def test_support_is_ignored_bitwise():
    x = _agent(dict(QDIST, v_min=-300.0, v_max=0.0))
    y = _agent(dict(QDIST, v_min=-7.0, v_max=1e6))
    for _ in range(3):
        assert x.train() == y.train()
    for net in ("actor", "critic", "actor_target", "critic_target"):
        sx, sy = getattr(x, net).state_dict(), getattr(y, net).state_dict()
        for k in sx:
            assert torch.equal(sx[k], sy[k]), (net, k)


def test_true_td_flag_is_accepted_and_inert():
    x = _agent(dict(QDIST), true_td_priorities=False)
    y = _agent(dict(QDIST), true_td_priorities=True)
    for _ in range(2):
        assert x.train() == y.train()
    assert np.array_equal(x.replayBuffer.state_dict()["leaves"],
                          y.replayBuffer.state_dict()["leaves"])


def test_invalid_kappa_refused_by_ddpg():
    for bad in (0.0, -0.5, float("nan")):
        with pytest.raises(ValueError):
            DDPG(3, 1, critic_dist_info=dict(QDIST, kappa=bad), hidden=16)


def test_state_dict_round_trip():
    x = _agent(dict(QDIST))
    x.train()
    st = x.state_dict()
    y = _agent(dict(QDIST), seed=9)
    y.load_state_dict(st)
    for net in ("actor", "critic", "actor_target", "critic_target"):
        sx, sy = getattr(x, net).state_dict(), getattr(y, net).state_dict()
        for k in sx:
            assert torch.equal(sx[k], sy[k]), (net, k)
    assert y.train_steps_done == x.train_steps_done
    assert np.array_equal(x.replayBuffer.state_dict()["leaves"],
                          y.replayBuffer.state_dict()["leaves"])
    assert np.isfinite(y.train()).all()


# ---------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------

def test_cli_flags():
    args = make_parser().parse_args([])
    assert args.critic_dist == "categorical" and args.huber_kappa == 1.0
    d = critic_dist_info(args)
    assert d["type"] == "categorical" and "kappa" not in d
    args = make_parser().parse_args(["--critic_dist", "quantile",
                                     "--huber_kappa", "0.5",
                                     "--n_atoms", "32"])
    d = critic_dist_info(args)
    assert d == {"type": "quantile", "v_min": args.v_min,
                 "v_max": args.v_max, "n_atoms": 32, "kappa": 0.5}
    agent = DDPG(3, 1, critic_dist_info=d, hidden=16)
    assert agent.dist_type == "quantile" and agent.kappa == 0.5
    assert agent.n_atoms == 32


@pytest.mark.parametrize("bad", ["0", "-1", "nan"])
def test_cli_refuses_invalid_kappa(bad, capsys):
    with pytest.raises(SystemExit):
        make_parser().parse_args(["--critic_dist", "quantile",
                                  "--huber_kappa", bad])
    capsys.readouterr()


def test_cli_refuses_unknown_dist(capsys):
    with pytest.raises(SystemExit):
        make_parser().parse_args(["--critic_dist", "mixture_of_gaussian"])
    capsys.readouterr()
