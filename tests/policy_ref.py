"""float64 numpy forward of the rollout-time policy evaluation (`PPO._act_core`, rsl_rl's
ActorCritic): normalise, the MLPs, a = mu + sigma * eps and the Gaussian log-probability.
Inputs are the fp32 values of the run under test, read exactly into float64."""

from __future__ import annotations

import numpy as np

_ACT = {"elu": lambda x: np.where(x > 0, x, np.expm1(np.minimum(x, 0))),
        "relu": lambda x: np.maximum(x, 0), "tanh": np.tanh}


def f64(t) -> np.ndarray:
  return t.detach().double().cpu().numpy()


def mlp64(x, seq, activation: str, normalizer):
  if hasattr(normalizer, "_mean"):
    x = (x - f64(normalizer._mean)) / (f64(normalizer._std) + normalizer.eps)
  linears = [m for m in seq if hasattr(m, "weight")]
  for i, lin in enumerate(linears):
    x = x @ f64(lin.weight).T + f64(lin.bias)
    if i + 1 < len(linears):
      x = _ACT[activation](x)
  return x


def act64(policy, activation: str, obs: dict, eps) -> dict:
  """actions, values, log_prob, mu, sigma of `policy` (an ActorCritic) on `obs` with the given
  standard normals, all float64 [N, .]."""
  mu = mlp64(f64(policy.get_actor_obs(obs)), policy.actor, activation, policy.actor_obs_normalizer)
  values = mlp64(f64(policy.get_critic_obs(obs)), policy.critic, activation, policy.critic_obs_normalizer)
  sigma = f64(policy.std) if policy.noise_std_type == "scalar" else np.exp(f64(policy.log_std))
  sigma = np.broadcast_to(sigma, mu.shape)
  actions = mu + sigma * f64(eps)
  logp = (-(actions - mu) ** 2 / (2 * sigma ** 2) - np.log(sigma) - 0.5 * np.log(2 * np.pi)).sum(-1, keepdims=True)
  return dict(actions=actions, values=values, log_prob=logp, mu=mu, sigma=sigma)
