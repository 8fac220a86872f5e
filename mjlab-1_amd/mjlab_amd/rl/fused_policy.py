"""Rollout-time policy evaluation as one HIP launch (`csrc/policy.hip`, `mjx_policy_act`).

`PPO._act_core` evaluates `ActorCritic` through torch: observation normalisation, two MLPs,
the Gaussian draw and its log-probability, some forty small kernels that `PPO._act_graphed`
replays as one graph.  `FusedPolicy` binds the same live parameters and normaliser buffers to
one kernel that carries 32 envs per workgroup through every layer with the activations in LDS
and the products on the matrix cores, and writes actions, values, log-probabilities, means and
standard deviations straight into the rows it is given (the rollout storage's row `t`).

The kernel's limits are checked here once, without a GPU: a feed-forward `ActorCritic`, at most
5 linear layers per network, inputs up to 1024 wide, hidden layers up to 512, up to 64 actions,
activation elu / relu / tanh.  Anything else is a `ValueError` naming the limit: there is no
torch fallback behind this class.
"""

from __future__ import annotations

import ctypes

import torch
import torch.nn as nn

from .._lib import check, lib

MAX_LAYERS, MAX_INPUT, MAX_HIDDEN, MAX_ACTIONS = 5, 1024, 512, 64
_ACTIVATION = {nn.ReLU: 1, nn.ELU: 2, nn.Tanh: 3}
_VP = ctypes.c_void_p


class PolicyNet(ctypes.Structure):
  """`mjxPolicyNet` (include/mjx355.h)."""
  _fields_ = [("nlayer", ctypes.c_int32), ("activation", ctypes.c_int32),
              ("width", ctypes.c_int32 * (MAX_LAYERS + 1)), ("obs_stride", ctypes.c_int32),
              ("norm_eps", ctypes.c_float), ("weight", _VP * MAX_LAYERS), ("bias", _VP * MAX_LAYERS),
              ("obs", _VP), ("norm_mean", _VP), ("norm_std", _VP)]


class PolicyDesc(ctypes.Structure):
  """`mjxPolicyDesc` (include/mjx355.h); `mjx_policy_desc_size` guards the layout."""
  _fields_ = ([("n", ctypes.c_int32), ("std_is_log", ctypes.c_int32), ("actor", PolicyNet),
               ("critic", PolicyNet), ("std", _VP), ("eps", _VP)]
              + [(k, _VP) for k in ("actions", "values", "log_prob", "mu", "sigma")]
              + [(k + "_stride", ctypes.c_int32) for k in ("actions", "values", "log_prob", "mu", "sigma")]
              + [("reserved", ctypes.c_int32)])


def _layers(seq: nn.Sequential, who: str, max_out: int):
  """The linear layers of an `mlp()` and its activation code, within the kernel's limits."""
  linears = [m for m in seq if isinstance(m, nn.Linear)]
  others = [m for m in seq if not isinstance(m, nn.Linear)]
  if not 1 <= len(linears) <= MAX_LAYERS:
    raise ValueError(f"FusedPolicy: {who} has {len(linears)} linear layers, the kernel takes 1 to {MAX_LAYERS}")
  code = 0
  for m in others:
    c = _ACTIVATION.get(type(m))
    if c is None or (c == 2 and m.alpha != 1.0):
      raise ValueError(f"FusedPolicy: {who} activation {type(m).__name__} is not one of elu (alpha 1), relu, tanh")
    if code not in (0, c):
      raise ValueError(f"FusedPolicy: {who} mixes activations, the kernel takes one per network")
    code = c
  if linears[0].in_features > MAX_INPUT:
    raise ValueError(f"FusedPolicy: {who} input width {linears[0].in_features} exceeds {MAX_INPUT}")
  for lin in linears[:-1]:
    if lin.out_features > MAX_HIDDEN:
      raise ValueError(f"FusedPolicy: {who} hidden width {lin.out_features} exceeds {MAX_HIDDEN}")
  if linears[-1].out_features > max_out:
    raise ValueError(f"FusedPolicy: {who} output width {linears[-1].out_features} exceeds {max_out}")
  if any(lin.bias is None for lin in linears):
    raise ValueError(f"FusedPolicy: {who} has a linear layer without a bias")
  return linears, code


class FusedPolicy:
  def __init__(self, policy):
    if getattr(policy, "is_recurrent", False):
      raise ValueError("FusedPolicy: recurrent policies are not supported (feed-forward ActorCritic only)")
    self.policy = policy
    self._actor, self._actor_act = _layers(policy.actor, "actor", MAX_ACTIONS)
    self._critic, self._critic_act = _layers(policy.critic, "critic", 1)
    self.num_actions = self._actor[-1].out_features
    self.launches = 0
    self._desc = None
    self._cat = {}  # concatenated observation rows of a network with several groups

  def _bind_net(self, net: PolicyNet, linears, code: int, normalizer) -> None:
    net.nlayer, net.activation = len(linears), code
    net.width[0] = linears[0].in_features
    for l, lin in enumerate(linears):
      if lin.weight.dtype != torch.float32 or not lin.weight.is_contiguous():
        raise ValueError("FusedPolicy: weights must be contiguous float32")
      net.width[l + 1] = lin.out_features
      net.weight[l], net.bias[l] = lin.weight.data_ptr(), lin.bias.data_ptr()
    if isinstance(normalizer, nn.Identity):
      net.norm_mean = net.norm_std = None
    else:  # EmpiricalNormalization updates these buffers in place
      net.norm_mean, net.norm_std = normalizer._mean.data_ptr(), normalizer._std.data_ptr()
      net.norm_eps = normalizer.eps

  def bind(self) -> None:
    """(Re)build the descriptor from the live parameters and normaliser buffers.  Their storage
    is what the kernel reads at every launch: in-place updates (the optimiser, the running
    normaliser, load_state_dict) need no new binding, moving the module to another device does."""
    p = self.policy
    std = p.std if p.noise_std_type == "scalar" else p.log_std
    if std.device.type != "cuda":
      raise RuntimeError("FusedPolicy runs on a GPU device (no CPU path)")
    L = lib()
    L.mjx_policy_desc_size.restype = ctypes.c_size_t
    if L.mjx_policy_desc_size() != ctypes.sizeof(PolicyDesc):
      raise RuntimeError("mjxPolicyDesc layout mismatch between include/mjx355.h and fused_policy.py")
    L.mjx_policy_act.argtypes = [ctypes.POINTER(PolicyDesc), _VP]
    d = PolicyDesc()
    self._bind_net(d.actor, self._actor, self._actor_act, p.actor_obs_normalizer)
    self._bind_net(d.critic, self._critic, self._critic_act, p.critic_obs_normalizer)
    d.std, d.std_is_log = std.data_ptr(), int(p.noise_std_type != "scalar")
    self._desc, self._ref, self._act, self._device = d, ctypes.byref(d), L.mjx_policy_act, std.device

  def _rows(self, obs: dict, group: str, net: PolicyNet) -> int:
    names = self.policy.obs_groups[group]
    if len(names) == 1:
      x = obs[names[0]]
    else:  # several groups: one row buffer of our own, refilled per call
      x = self._cat.get(group)
      parts = [obs[g] for g in names]
      if x is None or x.shape[0] != parts[0].shape[0]:
        x = self._cat[group] = torch.cat(parts, dim=-1)
      else:
        torch.cat(parts, dim=-1, out=x)
    if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1 or x.shape[1] != net.width[0]:
      raise ValueError(f"FusedPolicy: {group} observations must be float32 [N, {net.width[0]}] rows")
    net.obs, net.obs_stride = x.data_ptr(), x.stride(0)
    return x.shape[0]

  def _launch(self) -> None:
    stream = torch.cuda.current_stream(self._device).cuda_stream
    check(self._act(self._ref, _VP(stream)))
    self.launches += 1

  def act(self, obs: dict, eps, actions, values, log_prob, mu, sigma) -> None:
    """Evaluate both networks on `obs` and write a = mu + sigma * eps, the value, log p(a), mu
    and sigma into the given float32 [N, .] tensors (rows may be strided)."""
    if self._desc is None:
      self.bind()
    d = self._desc
    d.n = n = self._rows(obs, "policy", d.actor)
    self._rows(obs, "critic", d.critic)
    if eps.shape != (n, self.num_actions) or not eps.is_contiguous() or eps.dtype != torch.float32:
      raise ValueError(f"FusedPolicy: eps must be contiguous float32 [{n}, {self.num_actions}]")
    d.eps = eps.data_ptr()
    for name, t, w in (("actions", actions, self.num_actions), ("values", values, 1),
                       ("log_prob", log_prob, 1), ("mu", mu, self.num_actions),
                       ("sigma", sigma, self.num_actions)):
      if t.shape != (n, w) or t.dtype != torch.float32 or t.stride(1) != 1:
        raise ValueError(f"FusedPolicy: {name} must be float32 [{n}, {w}] rows")
      setattr(d, name, t.data_ptr())
      setattr(d, name + "_stride", t.stride(0))
    self._launch()

  def act_inference(self, obs: dict) -> torch.Tensor:
    """The action mean (ActorCritic.act_inference): the actor alone, no draw."""
    if self._desc is None:
      self.bind()
    d = self._desc
    d.n = n = self._rows(obs, "policy", d.actor)
    mu = torch.empty(n, self.num_actions, device=self._device)
    d.eps = d.actions = d.values = d.log_prob = d.sigma = None
    d.mu, d.mu_stride = mu.data_ptr(), self.num_actions
    self._launch()
    return mu
