"""The fused rollout policy kernel (`csrc/policy.hip` through `FusedPolicy`) against the float64
forward of `policy_ref.py`.

Yardstick: the fp32 torch eager path (`PPO._act_core` with the same standard normals) on the
same inputs.  For each of actions, values, log_prob, mu and sigma the fused result's max abs
error against fp64 must be at most 4 x the eager path's, plus a floor of eps32 * max|ref|:
the factor covers another, equally precise summation order and the factor-two scatter of a
maximum over so few samples.  Largest ratio err / (4 err_eager + floor) seen on an MI355X over
all cases below: 0.95 (the value of the lone row N = 1 of the G1 networks, relu, no normaliser:
2.6e-7 against a bound of 2.7e-7, two ulps of a single sample).

Rows: the kernel's row tile is 32, so N = 1 (a lone row), 33 (one past a tile) and 95 (a ragged
tail of three tiles).  Widths: one tile of everything; widths that are no multiple of any MFMA
edge; the shipped G1 networks.
"""

from __future__ import annotations

import types

import numpy as np
import pytest
import torch

from mjlab_amd.rl.fused_policy import FusedPolicy
from mjlab_amd.rl.ppo import PPO, ActorCritic
from mjlab_amd.rl.runner import OnPolicyRunner
from policy_ref import act64

pytestmark = pytest.mark.gpu
NAMES = ("actions", "values", "log_prob", "mu", "sigma")
SHAPES = {"tiny": (5, 7, (32,), 1), "odd": (99, 102, (48, 20), 12), "g1": (99, 111, (512, 256, 128), 29)}
EPS32 = float(np.finfo(np.float32).eps)


def make_policy(shape, activation, norm, noise, device, seed=0):
  na_in, nc_in, hidden, nact = SHAPES[shape]
  g = torch.Generator().manual_seed(seed)
  obs = {"policy": torch.zeros(1, na_in), "critic": torch.zeros(1, nc_in)}
  p = ActorCritic(obs, {"policy": ["policy"], "critic": ["critic"]}, nact, actor_obs_normalization=norm,
                  critic_obs_normalization=norm, actor_hidden_dims=hidden, critic_hidden_dims=hidden,
                  activation=activation, noise_std_type=noise)
  with torch.no_grad():
    for lin in [m for m in list(p.actor) + list(p.critic) if isinstance(m, torch.nn.Linear)]:
      lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) / lin.in_features ** 0.5)
      lin.bias.copy_(0.1 * torch.randn(lin.bias.shape, generator=g))
    sigma = 0.3 + 0.9 * torch.rand(nact, generator=g)
    (p.std if noise == "scalar" else p.log_std).copy_(sigma if noise == "scalar" else sigma.log())
    if norm:
      for nz in (p.actor_obs_normalizer, p.critic_obs_normalizer):
        nz._mean.copy_(torch.randn(nz._mean.shape, generator=g))
        nz._std.copy_(0.5 + 1.5 * torch.rand(nz._std.shape, generator=g))
  return p.to(device)


def draw(shape, n, device, seed):
  na_in, nc_in, _, nact = SHAPES[shape]
  g = torch.Generator().manual_seed(seed)
  obs = {"policy": 0.5 + 2 * torch.randn(n, na_in, generator=g), "critic": 0.5 + 2 * torch.randn(n, nc_in, generator=g)}
  return {k: v.to(device) for k, v in obs.items()}, torch.randn(n, nact, generator=g).to(device)


def check(tag, got: dict, policy, activation, obs, eps):
  """got[name] (fused) against fp64 within 4 x the eager fp32 path's own error + the floor."""
  ref = act64(policy, activation, obs, eps)
  with torch.no_grad():
    eager = dict(zip(NAMES, PPO(policy, device=eps.device)._act_core(obs, eps)))
  for k in NAMES:
    err = np.abs(got[k].double().cpu().numpy() - ref[k]).max()
    bound = 4 * np.abs(eager[k].double().cpu().numpy() - ref[k]).max() + EPS32 * np.abs(ref[k]).max()
    print(f"fused policy {tag} {k}: err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
    assert err <= bound, (tag, k, err, bound)


@pytest.mark.parametrize("noise", ["scalar", "log"])
@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("activation", ["elu", "relu", "tanh"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_fused_act_against_fp64(shape, activation, norm, noise, gpu_device):
  policy = make_policy(shape, activation, norm, noise, gpu_device)
  fused = FusedPolicy(policy)
  nact = SHAPES[shape][3]
  for n in (1, 33, 95):
    obs, eps = draw(shape, n, gpu_device, seed=n)
    # row t = 1 of a [3, 2 n, d] tensor, every second row: the rest must stay as it was
    bufs = {k: torch.full((3, 2 * n, 1 if k in ("values", "log_prob") else nact), 777.0, device=gpu_device)
            for k in NAMES}
    fused.act(obs, eps, *[bufs[k][1, ::2] for k in NAMES])
    check(f"{shape} {activation} norm={norm} {noise} n={n}", {k: bufs[k][1, ::2] for k in NAMES},
          policy, activation, obs, eps)
    for k in NAMES:
      assert (bufs[k][0] == 777.0).all() and (bufs[k][2] == 777.0).all() and (bufs[k][1, 1::2] == 777.0).all(), k
  assert fused.launches == 3


def test_ppo_act_writes_the_storage_rows(gpu_device):
  policy = make_policy("g1", "elu", True, "scalar", gpu_device)
  alg = PPO(policy, device=gpu_device, fused_act=True)
  obs0, _ = draw("g1", 64, gpu_device, seed=0)
  alg.init_storage(64, 4, obs0, 29)
  s = alg.storage
  for t in range(2):
    obs, _ = draw("g1", 64, gpu_device, seed=10 + t)
    actions = alg.act(obs)
    assert actions.data_ptr() == s.actions[t].data_ptr()
    got = dict(zip(NAMES, (s.actions[t], s.values[t], s.actions_log_prob[t], s.mu[t], s.sigma[t])))
    check(f"PPO.act t={t}", got, policy, "elu", obs, alg._feps.clone())
    assert torch.equal(s.observations["policy"][t], obs["policy"])
    s.step += 1
  assert alg._fused.launches == 2 and alg._act_graph is None
  assert not s.actions[2:].any() and not s.values[2:].any()


def test_inference_policy_is_mu(gpu_device):
  policy = make_policy("g1", "elu", True, "log", gpu_device)
  obs, eps = draw("g1", 33, gpu_device, seed=3)
  env = types.SimpleNamespace(num_envs=33, num_actions=29, get_observations=lambda: obs)
  cfg = dict(algorithm={}, obs_groups={"policy": ["policy"], "critic": ["critic"]}, num_steps_per_env=2,
             save_interval=0, policy=dict(actor_hidden_dims=(512, 256, 128), critic_hidden_dims=(512, 256, 128),
                                          actor_obs_normalization=True, critic_obs_normalization=True,
                                          noise_std_type="log"))
  runner = OnPolicyRunner(env, cfg, device=gpu_device)
  runner.alg.policy.load_state_dict(policy.state_dict())
  act = runner.get_inference_policy(fused=True)
  mu = act(obs)
  ref = act64(runner.alg.policy, "elu", obs, eps)["mu"]
  with torch.no_grad():
    eager = runner.alg.policy.act_inference(obs)
  err = np.abs(mu.double().cpu().numpy() - ref).max()
  bound = 4 * np.abs(eager.double().cpu().numpy() - ref).max() + EPS32 * np.abs(ref).max()
  print(f"fused inference mu: err {err:.3e} bound {bound:.3e}")
  assert mu.shape == (33, 29) and err <= bound
