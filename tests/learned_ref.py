"""fp64 reference of the learned (MLP) actuator with a running error bound, shared by
tests/test_learned_actuator.py (torch form, CPU) and tests/test_gpu_learned_actuator.py (engine).

The inputs are formed with the individually rounded fp32 operations both implementations use
(frame = fl(pt - q), qd; input = fl(frame * scale)), so they carry no error.  Each layer is
evaluated in fp64 next to a bound on the error of ANY fp32 evaluation of it (any summation
order, fused multiply-add or not), with u = 2^-24 and g(k) = k u / (1 - k u):

  pre-activation   e_a = |W| e_x + g(n_in + 1) (|W| (|x| + e_x) + |b|)
  activation phi   e   = e_a + k_phi u (|phi(a)| + e_a)      (all four are 1-Lipschitz)
                   k_relu = 0, k_softsign = 3 (one add, one correctly rounded division);
                   k_tanh / k_elu are measured against torch's own fp32 functions (measure_k)
  torque           e_t = |torque_scale| e + u |t|
  the DC-motor clip is 1-Lipschitz, its limits are fp32 operations restated exactly

and the assertion is |ctrl - ctrl_ref| <= e_t + u |ctrl_ref| elementwise (check)."""

import numpy as np
import torch
from torch import nn

U = 2.0 ** -24
F32 = np.float32
ACTS = {nn.ReLU: "relu", nn.Softsign: "softsign", nn.Tanh: "tanh", nn.ELU: "elu"}
K_FIXED = {"none": 0.0, "relu": 0.0, "softsign": 3.0}


def make_net(widths, act, seed, gain=1.5, out_gain=1.0):
  """A seeded `nn.Sequential` MLP: Linear layers of `widths` with `act` (an nn.Module class)
  between them, weights uniform on +-gain / sqrt(n_in) so that the activations are exercised;
  the last layer scaled by `out_gain`."""
  g = torch.Generator().manual_seed(seed)
  mods = []
  for l in range(len(widths) - 1):
    lin = nn.Linear(widths[l], widths[l + 1])
    with torch.no_grad():
      lin.weight.copy_((torch.rand(lin.weight.shape, generator=g) * 2 - 1) * gain / np.sqrt(widths[l]))
      lin.bias.copy_((torch.rand(lin.bias.shape, generator=g) * 2 - 1) * 0.3)
      if l + 2 == len(widths):
        lin.weight.mul_(out_gain)
        lin.bias.mul_(out_gain)
    mods.append(lin)
    if l + 2 < len(widths):
      mods.append(act())
  return nn.Sequential(*mods)


def save_net(seq, path):
  torch.jit.script(seq).save(str(path))
  return str(path)


def layers_of(seq):
  """[(W fp64 [out, in], b fp64 [out], activation name)] of an `nn.Sequential` MLP."""
  out = []
  for mod in seq:
    if isinstance(mod, nn.Linear):
      out.append([mod.weight.detach().double().numpy(), mod.bias.detach().double().numpy(), "none"])
    else:
      out[-1][2] = ACTS[type(mod)]
  return [tuple(l) for l in out]


def _phi(name, a):
  if name == "relu":
    return np.maximum(a, 0.0)
  if name == "softsign":
    return a / (1.0 + np.abs(a))
  if name == "tanh":
    return np.tanh(a)
  if name == "elu":
    return np.where(a > 0, a, np.expm1(np.minimum(a, 0.0)))
  return a


def measure_k(name, lo, hi, device="cpu", points=1 << 20):
  """k_tanh / k_elu: torch's fp32 function on `device` over a dense grid on [lo, hi] against
  fp64, the largest error in units of u |phi|, doubled (another valid fp32 implementation may
  err the other way), at least 2."""
  a = torch.linspace(lo, hi, points, dtype=torch.float64).float()
  a = a[a != 0]
  fn = torch.tanh if name == "tanh" else torch.nn.functional.elu
  got = fn(a.to(device)).double().cpu().numpy()
  want = _phi(name, a.double().numpy())
  k = float(np.max(np.abs(got - want) / (U * np.abs(want))))
  return max(2.0 * k, 2.0)


def pre_activation_range(layers, x32):
  """(lo, hi) over every pre-activation of `layers` on the inputs `x32`."""
  x = np.asarray(x32, dtype=np.float64)
  lo, hi = 0.0, 0.0
  for W, b, name in layers:
    a = x @ W.T + b
    if name != "none":
      lo, hi = min(lo, float(a.min())), max(hi, float(a.max()))
    x = _phi(name, a)
  return lo - 0.5, hi + 0.5


def inputs(pe, qd, pos_scale, vel_scale, order):
  """The network input `[..., 2 H]` (fp32) from the lag-indexed frames `pe`, `qd` `[..., H]`
  (fp32): each scaled by one fp32 multiplication, concatenated in `order`."""
  assert pe.dtype == F32 and qd.dtype == F32
  p = pe * F32(pos_scale)
  v = qd * F32(vel_scale)
  return np.concatenate([p, v] if order == "pos_vel" else [v, p], axis=-1)


def evaluate(layers, x32, k_act):
  """(y, e): the network's output on fp32 inputs `[..., n_in]` in fp64 and the bound."""
  x = np.asarray(x32, dtype=np.float64)
  e = np.zeros_like(x)
  for W, b, name in layers:
    k = W.shape[1] + 1
    g = k * U / (1 - k * U)
    aW = np.abs(W)
    a = x @ W.T + b
    ea = e @ aW.T + g * ((np.abs(x) + e) @ aW.T + np.abs(b))
    x = _phi(name, a)
    kphi = K_FIXED[name] if name in K_FIXED else k_act[name]
    e = ea + kphi * U * (np.abs(x) + ea)
  return x[..., 0], e[..., 0]


def dc_limits(qd, flim, sat, vlim):
  """(lo, hi) of DcMotorActuator._clip_effort in its fp32 operations (each rounded once; the
  corner velocity as `initialize` computes it)."""
  qd, flim, sat, vlim = (np.asarray(v, dtype=F32) for v in (qd, flim, sat, vlim))
  vc = vlim * (F32(1) + flim / sat)
  r = np.clip(qd, -vc, vc) / vlim
  hi = np.minimum(sat * (F32(1) - r), flim)
  lo = np.maximum(sat * (F32(-1) - r), -flim)
  return lo.astype(np.float64), hi.astype(np.float64)


def ctrl_ref(layers, pe, qd, cfg, k_act, order=None):
  """(ctrl, bound, clipped) of a learned actuator with `cfg` (pos_scale, vel_scale, torque_scale,
  input_order, effort_limit, saturation_effort, velocity_limit) on lag-indexed fp32 frames
  `pe`, `qd` `[..., H]`; `clipped`: where the DC clip binds."""
  x = inputs(pe, qd, cfg.pos_scale, cfg.vel_scale, order or cfg.input_order)
  y, e = evaluate(layers, x, k_act)
  ts = float(F32(cfg.torque_scale))
  t = y * ts
  et = abs(ts) * e + U * np.abs(t)
  lo, hi = dc_limits(qd[..., 0], cfg.effort_limit, cfg.saturation_effort, cfg.velocity_limit)
  c = np.minimum(np.maximum(t, lo), hi)
  return c, et + U * np.abs(c), (t < lo) | (t > hi)


def check(got, ref, bound, what=""):
  """Assert |got - ref| <= bound elementwise; prints and returns the largest err / bound."""
  err = np.abs(np.asarray(got, dtype=np.float64) - ref)
  ratio = float(np.max(err / np.maximum(bound, 1e-300)))
  print(f"{what}: largest err / bound = {ratio:.3f} (largest err {float(err.max()):.3e})")
  assert (err <= bound).all(), f"{what}: err / bound = {ratio}"
  return ratio


def differs(got, ref, bound):
  """Fraction of elements where `got` is further than the bound from `ref`."""
  return float(np.mean(np.abs(np.asarray(got, dtype=np.float64) - ref) > bound))


class History:
  """Host mirror of the torch path's history: per row the last H frames, lag-indexed
  (`pe[..., 0]` newest).  The first frame after a reset fills every lag (backfill)."""

  def __init__(self, n, nj, H):
    self.pe = np.zeros((n, nj, H), dtype=F32)
    self.qd = np.zeros((n, nj, H), dtype=F32)
    self.count = np.zeros(n, dtype=np.int64)

  def append(self, pe, qd, rows=None):
    rows = np.ones(len(self.count), bool) if rows is None else np.asarray(rows, bool)
    for buf, new in ((self.pe, pe), (self.qd, qd)):
      new = np.asarray(new, dtype=F32)
      shifted = np.concatenate([new[..., None], buf[..., :-1]], axis=-1)
      filled = np.repeat(new[..., None], buf.shape[-1], axis=-1)
      fresh = (self.count == 0)[:, None, None]
      buf[rows] = np.where(fresh, filled, shifted)[rows]
    self.count[rows] += 1

  def reset(self, rows):
    self.pe[rows] = 0
    self.qd[rows] = 0
    self.count[rows] = 0
