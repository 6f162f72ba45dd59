"""Quantile-regression critic loss (QR-DQN's loss on D4PG's critic).

The critic's K outputs are the values of K fixed quantiles, theta_i at
``tau_i = (2i + 1) / (2K)``; there is no support and no projection.  For one
batch row with target samples ``T_j = r + gamma_n * (1 - done) * theta'_j``
(``theta'`` the target critic's quantiles at the target actor's action):

    u_ij   = T_j - theta_i
    H(u)   = 0.5 u^2                     if |u| <= kappa
             kappa * (|u| - 0.5 kappa)   otherwise
    rho_ij = |tau_i - 1{u_ij < 0}| * H(u_ij) / kappa
    l      = (1/K) * sum_i sum_j rho_ij

so that d l / d theta_i = -(1/K) sum_j |tau_i - 1{u_ij < 0}| *
clip(u_ij, -kappa, kappa) / kappa, which is what autograd gives below and what
the HIP engine computes per row (ops/hip/engine_rowmath.hip, qr_grad_row).
"""

from __future__ import annotations

import torch


def quantile_taus(n_quantiles: int, device=None,
                  dtype=torch.float32) -> torch.Tensor:
    """The fixed quantile midpoints tau_i = (2i + 1) / (2K), [K]."""
    i = torch.arange(n_quantiles, device=device, dtype=dtype)
    return (2.0 * i + 1.0) / (2.0 * n_quantiles)


def quantile_targets(next_quantiles: torch.Tensor, rewards: torch.Tensor,
                     dones: torch.Tensor, gamma_n: float) -> torch.Tensor:
    """Target samples T = r + gamma_n * (1 - done) * theta', [B, K]."""
    B = next_quantiles.shape[0]
    dtype = next_quantiles.dtype
    r = rewards.reshape(B, 1).to(dtype)
    d = dones.reshape(B, 1).to(dtype)
    return r + gamma_n * (1.0 - d) * next_quantiles


def quantile_huber_loss(theta: torch.Tensor, target: torch.Tensor,
                        kappa: float = 1.0) -> torch.Tensor:
    """Per-row quantile-Huber loss l_b, [B].

    Args:
      theta:  online quantiles, [B, K] (gradients flow into it).
      target: target samples T, [B, K'] (treated as constants; K' = K in the
              learner, any K' is accepted).
      kappa:  Huber threshold, > 0.
    """
    if not kappa > 0.0:
        raise ValueError("kappa must be > 0, got %r" % (kappa,))
    K = theta.shape[1]
    tau = quantile_taus(K, device=theta.device, dtype=theta.dtype)
    u = target.detach().unsqueeze(1) - theta.unsqueeze(2)       # [B, i, j]
    au = u.abs()
    huber = torch.where(au <= kappa, 0.5 * u * u,
                        kappa * (au - 0.5 * kappa))
    weight = (tau.reshape(1, K, 1) - (u.detach() < 0).to(theta.dtype)).abs()
    return (weight * huber / kappa).sum(dim=(1, 2)) / K
