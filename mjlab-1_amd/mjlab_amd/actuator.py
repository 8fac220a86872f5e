"""Explicit actuators: ideal PD, DC motor, the learned MLP and the delay wrapper.

Restates `src/mjlab/actuator/{actuator,pd_actuator,dc_actuator,delayed_actuator,
learned_actuator}.py` with
the reference's class names, cfg fields and defaults.  An explicit actuator computes its
torque outside the model's own actuation and writes it to a `<motor>`:

- `IdealPdActuator`: `clamp(kp (pt - q) + kd (vt - qd) + ff, +-effort_limit)`, the gains
  and the limit per env and joint (`set_gains`, `set_effort_limit`).
- `DcMotorActuator`: the same law, clipped by the torque-speed line from `saturation_effort`
  at rest to zero at `velocity_limit`, then by `effort_limit`.
- `LearnedMlpActuator`: a TorchScript network maps the last `history_length` frames of
  (position error, joint velocity) of a joint to its torque, which the DC-motor clip bounds.
- `DelayedActuator`: wraps any of them and reads its targets `lag` physics steps late
  (`mjlab_amd.buffers.DelayBuffer`).

The compiler sees the group each cfg compiles to (`compile_group`: a `MotorActuatorGroup`
with `ctrlrange = forcerange = +-effort_limit`); the runtime objects are built by
`scene.Entity` after the scene is compiled.  `Simulation.set_explicit_actuators` hands the
ideal-PD and DC laws, and a learned actuator whose module is a plain MLP (`extract_mlp`), to
the engine's phase A (engine mode: the per-env tensors of these objects are the engine's own
inputs, so the setters act on it without a copy); otherwise `Entity.write_data_to_sim`
evaluates `compute` in torch, which runs any TorchScript module.  The XML actuators of the
reference are not implemented.
"""

from __future__ import annotations

import ctypes
import warnings
from dataclasses import dataclass, field

import torch

from .buffers import CircularBuffer, DelayBuffer
from .compiler.model import MotorActuatorGroup, PositionActuatorGroup, VelocityActuatorGroup

# engine kinds (include/mjx355.h, mjxActuatorDesc.kind)
KIND_BUILTIN, KIND_DELAYED, KIND_IDEAL_PD, KIND_DC_MOTOR = 0, 1, 2, 3


@dataclass(kw_only=True)
class ActuatorCfg:
  """`actuator/actuator.py:17-49`."""
  joint_names_expr: tuple[str, ...]
  armature: float = 0.0
  frictionloss: float = 0.0

  def build(self, entity, joint_ids: list[int], joint_names: list[str]) -> "Actuator":
    raise NotImplementedError

  def compile_group(self) -> MotorActuatorGroup:
    """What `edit_spec` adds to the model: the builtin group the scene compiler emits."""
    raise NotImplementedError


@dataclass
class ActuatorCmd:
  """Targets and joint state of one actuator group, each `[num_envs, num_joints]`."""
  position_target: torch.Tensor
  velocity_target: torch.Tensor
  effort_target: torch.Tensor
  joint_pos: torch.Tensor
  joint_vel: torch.Tensor


class Actuator:
  """`actuator/actuator.py:72-175`.  `joint_ids` index the entity's joints, `ctrl_ids` the
  entity's actuators (`EntityData.write_ctrl` maps them to the model's)."""

  def __init__(self, entity, joint_ids: list[int], joint_names: list[str]) -> None:
    self.entity = entity
    self._joint_ids_list = list(joint_ids)
    self._joint_names = list(joint_names)
    self._ctrl_ids_list: list[int] = []
    self._joint_ids: torch.Tensor | None = None
    self._ctrl_ids: torch.Tensor | None = None

  @property
  def joint_ids(self) -> torch.Tensor:
    assert self._joint_ids is not None
    return self._joint_ids

  @property
  def joint_names(self) -> list[str]:
    return self._joint_names

  @property
  def ctrl_ids(self) -> torch.Tensor:
    assert self._ctrl_ids is not None
    return self._ctrl_ids

  def edit_spec(self, spec=None, joint_names=None) -> MotorActuatorGroup:
    """The group this actuator adds to the model.  The scene compiler applies it (one
    `<motor>` per joint, armature on the joint); `spec` is accepted for the reference's
    signature and not edited."""
    raise NotImplementedError

  def initialize(self, mj_model, model, data, device: str) -> None:
    self._joint_ids = torch.tensor(self._joint_ids_list, dtype=torch.long, device=device)
    self._ctrl_ids = torch.tensor(self._ctrl_ids_list, dtype=torch.long, device=device)

  def compute(self, cmd: ActuatorCmd) -> torch.Tensor:
    raise NotImplementedError

  def reset(self, env_ids=None) -> None:
    pass

  def reset_masked(self, mask: torch.Tensor) -> None:
    pass

  def update(self, dt: float) -> None:
    pass


def _num_worlds(data) -> int:
  n = getattr(data, "nworld", None)
  return int(n) if n is not None else int(data.qpos.shape[0])


@dataclass(kw_only=True)
class IdealPdActuatorCfg(ActuatorCfg):
  """`actuator/pd_actuator.py:21-35`."""
  stiffness: float
  damping: float
  effort_limit: float = float("inf")

  def build(self, entity, joint_ids, joint_names) -> "IdealPdActuator":
    return IdealPdActuator(self, entity, joint_ids, joint_names)

  def compile_group(self) -> MotorActuatorGroup:
    return MotorActuatorGroup(tuple(self.joint_names_expr), effort_limit=self.effort_limit,
                              armature=self.armature, frictionloss=self.frictionloss)


class IdealPdActuator(Actuator):
  """`actuator/pd_actuator.py:38-150`."""
  engine_kind = KIND_IDEAL_PD

  def __init__(self, cfg, entity, joint_ids, joint_names) -> None:
    super().__init__(entity, joint_ids, joint_names)
    self.cfg = cfg
    self.stiffness: torch.Tensor | None = None
    self.damping: torch.Tensor | None = None
    self.force_limit: torch.Tensor | None = None
    self.default_stiffness: torch.Tensor | None = None
    self.default_damping: torch.Tensor | None = None
    self.default_force_limit: torch.Tensor | None = None

  def edit_spec(self, spec=None, joint_names=None) -> MotorActuatorGroup:
    return self.cfg.compile_group()

  def _full(self, n: int, value: float, device: str) -> torch.Tensor:
    return torch.full((n, len(self._joint_names)), float(value), dtype=torch.float32, device=device)

  def initialize(self, mj_model, model, data, device: str) -> None:
    super().initialize(mj_model, model, data, device)
    n = _num_worlds(data)
    self.stiffness = self._full(n, self.cfg.stiffness, device)
    self.damping = self._full(n, self.cfg.damping, device)
    self.force_limit = self._full(n, self.cfg.effort_limit, device)
    self.default_stiffness = self.stiffness.clone()
    self.default_damping = self.damping.clone()
    self.default_force_limit = self.force_limit.clone()

  def compute(self, cmd: ActuatorCmd) -> torch.Tensor:
    # the engine's phase A runs these operations in this order, each rounded once
    pos_error = cmd.position_target - cmd.joint_pos
    vel_error = cmd.velocity_target - cmd.joint_vel
    torque = self.stiffness * pos_error
    torque = torque + self.damping * vel_error
    torque = torque + cmd.effort_target
    return self._clip_effort(torque, cmd)

  def _clip_effort(self, effort: torch.Tensor, cmd: ActuatorCmd | None = None) -> torch.Tensor:
    return torch.clamp(effort, -self.force_limit, self.force_limit)

  def set_gains(self, env_ids, kp: torch.Tensor | None = None, kd: torch.Tensor | None = None) -> None:
    """Per-env gains, `[len(env_ids), num_joints]` or `[len(env_ids)]`."""
    if kp is not None:
      self.stiffness[env_ids] = kp.unsqueeze(-1) if kp.ndim == 1 else kp
    if kd is not None:
      self.damping[env_ids] = kd.unsqueeze(-1) if kd.ndim == 1 else kd

  def set_effort_limit(self, env_ids, effort_limit: torch.Tensor) -> None:
    if effort_limit.ndim == 1:
      effort_limit = effort_limit.unsqueeze(-1)
    self.force_limit[env_ids] = effort_limit


@dataclass(kw_only=True)
class DcMotorActuatorCfg(IdealPdActuatorCfg):
  """`actuator/dc_actuator.py:25-70`: `saturation_effort` is the stall torque,
  `velocity_limit` the no-load speed; `effort_limit` is the continuous rating."""
  saturation_effort: float
  velocity_limit: float

  def __post_init__(self) -> None:
    if self.effort_limit == float("inf"):
      warnings.warn(
          "effort_limit is set to inf for DcMotorActuator, which creates an unrealistic motor "
          "with unlimited continuous torque. Consider setting effort_limit to your motor's "
          "continuous rating (<= saturation_effort). Use IdealPdActuator if you truly want "
          "unlimited torque.", UserWarning, stacklevel=2)
    if self.effort_limit > self.saturation_effort:
      warnings.warn(
          f"effort_limit ({self.effort_limit}) exceeds saturation_effort "
          f"({self.saturation_effort}). For realistic motors, continuous torque should be <= "
          "peak torque.", UserWarning, stacklevel=2)

  def build(self, entity, joint_ids, joint_names) -> "DcMotorActuator":
    return DcMotorActuator(self, entity, joint_ids, joint_names)


class DcMotorActuator(IdealPdActuator):
  """`actuator/dc_actuator.py:73-162`.  The corner velocity (where the torque-speed line
  meets `effort_limit`) is fixed at `initialize`, as in the reference."""
  engine_kind = KIND_DC_MOTOR

  def __init__(self, cfg, entity, joint_ids, joint_names) -> None:
    super().__init__(cfg, entity, joint_ids, joint_names)
    self.saturation_effort: torch.Tensor | None = None
    self.velocity_limit_motor: torch.Tensor | None = None
    self._vel_at_effort_lim: torch.Tensor | None = None

  def initialize(self, mj_model, model, data, device: str) -> None:
    super().initialize(mj_model, model, data, device)
    n = _num_worlds(data)
    self.saturation_effort = self._full(n, self.cfg.saturation_effort, device)
    self.velocity_limit_motor = self._full(n, self.cfg.velocity_limit, device)
    self._vel_at_effort_lim = self.velocity_limit_motor * (1 + self.force_limit / self.saturation_effort)

  def _clip_effort(self, effort: torch.Tensor, cmd: ActuatorCmd | None = None) -> torch.Tensor:
    vel = torch.clamp(cmd.joint_vel, min=-self._vel_at_effort_lim, max=self._vel_at_effort_lim)
    ratio = vel / self.velocity_limit_motor
    top = self.saturation_effort * (1.0 - ratio)
    bottom = self.saturation_effort * (-1.0 - ratio)
    max_effort = torch.clamp(top, max=self.force_limit)
    min_effort = torch.clamp(bottom, min=-self.force_limit)
    return torch.clamp(effort, min=min_effort, max=max_effort)


_INPUT_ORDERS = ("pos_vel", "vel_pos")


@dataclass(kw_only=True)
class LearnedMlpActuatorCfg(DcMotorActuatorCfg):
  """`actuator/learned_actuator.py:20-67`: `network_file` is a TorchScript file mapping
  `[rows, 2 * history_length]` to `[rows, 1]`; the PD gains are unused."""
  network_file: str
  pos_scale: float
  vel_scale: float
  torque_scale: float
  input_order: str = "pos_vel"
  history_length: int = 3
  stiffness: float = 0.0
  damping: float = 0.0

  def build(self, entity, joint_ids, joint_names) -> "LearnedMlpActuator":
    return LearnedMlpActuator(self, entity, joint_ids, joint_names)


class LearnedMlpActuator(DcMotorActuator):
  """`actuator/learned_actuator.py:70-207`, plus the row mask of `compute` (as
  `DelayedActuator.compute`): rows outside it keep their history and return the torque of
  their last evaluation."""
  takes_mask = True

  def __init__(self, cfg, entity, joint_ids, joint_names) -> None:
    super().__init__(cfg, entity, joint_ids, joint_names)
    if cfg.input_order not in _INPUT_ORDERS:
      raise ValueError(f"Invalid input order: {cfg.input_order}. Must be 'pos_vel' or 'vel_pos'.")
    self.network = None
    self._pos_error_history: CircularBuffer | None = None
    self._vel_history: CircularBuffer | None = None
    self._last: torch.Tensor | None = None  # [num_envs, num_joints] the last torque per row
    self._engine = None  # (EngineActuators, columns) while the engine holds the history
    self._mlp = None     # extract_mlp(self.network, history_length), cached

  def initialize(self, mj_model, model, data, device: str) -> None:
    super().initialize(mj_model, model, data, device)
    self.network = torch.jit.load(self.cfg.network_file, map_location=device)
    self.network.eval()
    n = _num_worlds(data)
    self._pos_error_history = CircularBuffer(self.cfg.history_length, n, device)
    self._vel_history = CircularBuffer(self.cfg.history_length, n, device)
    self._last = torch.zeros(n, len(self._joint_names), dtype=torch.float32, device=device)

  @property
  def mlp(self):
    """`extract_mlp` of the loaded module: `(MlpSpec | None, reason | None)`."""
    if self._mlp is None:
      self._mlp = extract_mlp(self.network, self.cfg.history_length)
    return self._mlp

  def compute(self, cmd: ActuatorCmd, mask: torch.Tensor | None = None) -> torch.Tensor:
    c, H = self.cfg, self.cfg.history_length
    pos_error = cmd.position_target - cmd.joint_pos
    self._pos_error_history.append(pos_error, mask)
    self._vel_history.append(cmd.joint_vel, mask)
    n, nj = cmd.joint_pos.shape
    pos = torch.stack([self._pos_error_history[lag] for lag in range(H)], dim=2).reshape(n * nj, H)
    vel = torch.stack([self._vel_history[lag] for lag in range(H)], dim=2).reshape(n * nj, H)
    pos, vel = pos * c.pos_scale, vel * c.vel_scale
    x = torch.cat([pos, vel] if c.input_order == "pos_vel" else [vel, pos], dim=1)
    with torch.inference_mode():
      torque = self.network(x)
    torque = torque.reshape(n, nj).clone() * c.torque_scale
    out = self._clip_effort(torque, cmd)
    if mask is not None:
      out = torch.where(mask.view(-1, 1), out, self._last)
    self._last.copy_(out)
    return out

  def reset(self, env_ids=None) -> None:
    if self._engine is not None:
      self._engine[0].reset_net_rows(self._engine[1], env_ids=env_ids)
      return
    if isinstance(env_ids, slice):
      env_ids = list(range(*env_ids.indices(self._pos_error_history.batch_size)))
    self._pos_error_history.reset(env_ids)
    self._vel_history.reset(env_ids)

  def reset_masked(self, mask: torch.Tensor) -> None:
    if self._engine is not None:
      self._engine[0].reset_net_rows(self._engine[1], mask=mask.bool())
      return
    self._pos_error_history.reset_masked(mask.bool())
    self._vel_history.reset_masked(mask.bool())


# ---------------------------------------------------------------------------------------------
# a TorchScript module as a plain MLP (the form the engine evaluates)

ACT_NONE, ACT_RELU, ACT_SOFTSIGN, ACT_TANH, ACT_ELU = 0, 1, 2, 3, 4  # csrc/engine.h kNet*
_ACT_CODES = {"ReLU": ACT_RELU, "Softsign": ACT_SOFTSIGN, "Tanh": ACT_TANH, "ELU": ACT_ELU}
MAX_NET_LAYERS, MAX_NET_WIDTH, MAX_NET_HISTORY, MAX_NETS = 4, 32, 8, 4  # csrc/engine.h
# Rounding errors of an fp32 activation in units of u |phi(a)|, u = 2^-24: exact for relu; one
# add and one correctly rounded division for softsign; tanh and elu are measured (act_ulps)
_ACT_ULPS = {ACT_NONE: 0.0, ACT_RELU: 0.0, ACT_SOFTSIGN: 3.0}


@dataclass
class MlpSpec:
  """Linear layers `weights[l]` `[out, in]` / `biases[l]` `[out]` (fp32, CPU, as torch stores
  them) with `activations[l]` after layer l (`ACT_*`; `ACT_NONE` after the last)."""
  weights: list
  biases: list
  activations: list

  @property
  def widths(self) -> list[int]:
    return [int(self.weights[0].shape[1])] + [int(w.shape[0]) for w in self.weights]

  def key(self) -> bytes:
    """Equal for equal networks (identical files share one engine network)."""
    parts = [bytes(self.activations)]
    for w, b in zip(self.weights, self.biases):
      parts += [w.numpy().tobytes(), b.numpy().tobytes()]
    return b"|".join(parts)


def _apply_act(code: int, a: torch.Tensor) -> torch.Tensor:
  if code == ACT_RELU:
    return a.clamp_min(0)
  if code == ACT_SOFTSIGN:
    return a / (1 + a.abs())
  if code == ACT_TANH:
    return torch.tanh(a)
  if code == ACT_ELU:
    return torch.where(a > 0, a, torch.expm1(a))
  return a


def act_ulps(code: int, lo: float, hi: float, device="cpu", points: int = 1 << 16) -> float:
  """k of the bound for activation `code`: fixed for none / relu / softsign; for tanh and elu
  torch's own fp32 function on `device` over a dense grid on [lo, hi] against fp64, the largest
  error in units of u |phi|, doubled (another valid fp32 implementation may err the other way),
  at least 2 -- as the tests' reference measures it."""
  if code in _ACT_ULPS:
    return _ACT_ULPS[code]
  a = torch.linspace(lo, hi, points, dtype=torch.float64).float()
  a = a[a != 0]
  fn = torch.tanh if code == ACT_TANH else torch.nn.functional.elu
  got = fn(a.to(device)).double().cpu()
  want = _apply_act(code, a.double())
  k = float(((got - want).abs() / (2.0 ** -24 * want.abs())).max())
  return max(2.0 * k, 2.0)


def mlp_eval_fp64(spec: MlpSpec, x: torch.Tensor, device="cpu"):
  """`spec` on fp32 inputs `x` `[rows, in]` in fp64, with a bound on the error of any fp32
  evaluation of the same layers (any summation order, fused or not): per layer, with
  g(k) = k u / (1 - k u), `e_a = |W| e_x + g(n_in + 1) (|W| (|x| + e_x) + |b|)`, and after a
  1-Lipschitz activation `e = e_a + k u (|phi(a)| + e_a)`, k from `act_ulps` on the layer's
  own pre-activation range (`device`: where the fp32 evaluation under test runs).  Returns
  `(y, e)`, `[rows, 1]`."""
  u = 2.0 ** -24
  x = x.double().cpu()
  e = torch.zeros_like(x)
  for w, b, code in zip(spec.weights, spec.biases, spec.activations):
    w, b = w.double(), b.double()
    k = w.shape[1] + 1
    g = k * u / (1 - k * u)
    a = x @ w.T + b
    ea = e @ w.abs().T + g * ((x.abs() + e) @ w.abs().T + b.abs())
    x = _apply_act(code, a)
    k_act = act_ulps(code, float(a.min()) - 0.5, float(a.max()) + 0.5, device)
    e = ea + k_act * u * (x.abs() + ea)
  return x, e


def extract_mlp(module, history_length: int):
  """`(MlpSpec, None)` where the TorchScript `module` is a plain MLP the engine can evaluate,
  else `(None, reason)`: a flat sequence of children named (`original_name`, which scripting
  and tracing an `nn.Sequential` both keep) `Linear` with a bias or `ReLU` / `Softsign` /
  `Tanh` / `ELU` (alpha 1); at most 4 linear layers, every width at most 32, `2 *
  history_length` inputs with `history_length <= 8`, one output, no activation after the last
  layer.  The result is checked against the module's own output on seeded inputs."""
  if history_length < 1 or history_length > MAX_NET_HISTORY:
    return None, f"history_length {history_length} (the engine holds 1 to {MAX_NET_HISTORY} frames)"
  weights, biases, acts = [], [], []
  children = list(module.children())
  if not children:
    return None, "the module has no child layers (a flat nn.Sequential is expected)"
  for child in children:
    name = getattr(child, "original_name", type(child).__name__)
    if name == "Linear":
      if len(weights) > len(acts):
        acts.append(ACT_NONE)
      bias = getattr(child, "bias", None)
      if bias is None:
        return None, "a Linear layer without a bias"
      weights.append(child.weight.detach().float().cpu().contiguous())
      biases.append(bias.detach().float().cpu().contiguous())
    elif name in _ACT_CODES:
      if len(weights) != len(acts) + 1:
        return None, f"{name} does not follow a Linear layer"
      alpha = getattr(child, "alpha", 1.0)
      if name == "ELU" and float(alpha) != 1.0:
        return None, f"ELU with alpha {float(alpha)} (the engine evaluates alpha 1)"
      acts.append(_ACT_CODES[name])
    else:
      return None, f"layer {name} (the engine evaluates Linear, ReLU, Softsign, Tanh and ELU)"
  if not weights:
    return None, "the module has no Linear layer"
  if len(acts) == len(weights):
    return None, "an activation after the last layer"
  acts.append(ACT_NONE)
  if len(weights) > MAX_NET_LAYERS:
    return None, f"{len(weights)} linear layers (at most {MAX_NET_LAYERS})"
  spec = MlpSpec(weights, biases, acts)
  widths = spec.widths
  for l, w in enumerate(weights):
    if w.ndim != 2 or biases[l].shape != (w.shape[0],) or w.shape[1] != widths[l]:
      return None, "layer shapes do not chain"
  if max(widths) > MAX_NET_WIDTH:
    return None, f"width {max(widths)} (at most {MAX_NET_WIDTH})"
  if widths[0] != 2 * history_length:
    return None, f"input width {widths[0]} is not 2 * history_length = {2 * history_length}"
  if widths[-1] != 1:
    return None, f"output width {widths[-1]} (one torque per joint is expected)"
  # the extraction checks itself: the layers against the module on seeded inputs
  gen = torch.Generator().manual_seed(20240229)
  x = (torch.rand(256, widths[0], generator=gen) * 2 - 1) * 2.0
  dev = children[0].weight.device if hasattr(children[0], "weight") else "cpu"
  with torch.inference_mode():
    got = module(x.to(dev)).double().cpu().reshape(-1, 1)
  want, err = mlp_eval_fp64(spec, x, dev)
  u = 2.0 ** -24
  if got.shape != want.shape or not bool(((got - want).abs() <= err + u * want.abs()).all()):
    return None, "the module is not the plain MLP its layers describe"
  return spec, None


class BuiltinActuator(Actuator):
  """A builtin actuator group behind a delay (`actuator/builtin_actuator.py`): the model's own
  <position> / <velocity> / <motor> computes the force, `compute` passes the matching target
  through as its ctrl."""
  _TARGET = ((PositionActuatorGroup, "position_target"), (VelocityActuatorGroup, "velocity_target"),
             (MotorActuatorGroup, "effort_target"))

  def __init__(self, cfg, entity, joint_ids, joint_names) -> None:
    super().__init__(entity, joint_ids, joint_names)
    self.cfg = cfg
    self._target = next((t for c, t in self._TARGET if isinstance(cfg, c)), None)
    if self._target is None:
      raise TypeError(f"DelayedActuatorCfg: unsupported base_cfg {type(cfg).__name__}")
    # the engine's delayed pass-through reads the position target
    self.engine_kind = KIND_DELAYED if self._target == "position_target" else None

  def edit_spec(self, spec=None, joint_names=None):
    return self.cfg

  def compute(self, cmd: ActuatorCmd) -> torch.Tensor:
    return getattr(cmd, self._target)


_DELAY_TARGETS = ("position", "velocity", "effort")


@dataclass(kw_only=True)
class DelayedActuatorCfg(ActuatorCfg):
  """`actuator/delayed_actuator.py:19-66`: lags count physics steps, not env steps."""
  joint_names_expr: tuple[str, ...] = field(init=False, default=())
  base_cfg: ActuatorCfg | PositionActuatorGroup | VelocityActuatorGroup | MotorActuatorGroup
  delay_target: str | tuple[str, ...] = "position"
  delay_min_lag: int = 0
  delay_max_lag: int = 0
  delay_hold_prob: float = 0.0
  delay_update_period: int = 0
  delay_per_env_phase: bool = True

  def __post_init__(self) -> None:
    self.joint_names_expr = tuple(self.base_cfg.joint_names_expr)
    self.armature = self.base_cfg.armature
    self.frictionloss = self.base_cfg.frictionloss
    for t in self.targets:
      if t not in _DELAY_TARGETS:
        raise ValueError(f"delay_target {t!r}: one of {_DELAY_TARGETS}")

  @property
  def targets(self) -> tuple[str, ...]:
    return (self.delay_target,) if isinstance(self.delay_target, str) else tuple(self.delay_target)

  def build(self, entity, joint_ids, joint_names) -> "DelayedActuator":
    if isinstance(self.base_cfg, ActuatorCfg):
      return DelayedActuator(self, self.base_cfg.build(entity, joint_ids, joint_names))
    return DelayedActuator(self, BuiltinActuator(self.base_cfg, entity, joint_ids, joint_names))

  def compile_group(self):
    """The base cfg's group; a builtin group is its own."""
    return self.base_cfg.compile_group() if isinstance(self.base_cfg, ActuatorCfg) else self.base_cfg


class DelayedActuator(Actuator):
  """`actuator/delayed_actuator.py:69-172`, plus the row mask of `compute` (below)."""
  takes_mask = True

  def __init__(self, cfg: DelayedActuatorCfg, base_actuator: Actuator) -> None:
    super().__init__(base_actuator.entity, base_actuator._joint_ids_list, base_actuator._joint_names)
    self.cfg = cfg
    self._base_actuator = base_actuator
    self._delay_buffers: dict[str, DelayBuffer] = {}
    self._engine = None  # (EngineActuators, columns) while the engine holds the delay state
    self._hold: torch.Tensor | None = None  # [num_envs] bool: rows whose lag set_lags pinned

  @property
  def base_actuator(self) -> Actuator:
    return self._base_actuator

  def edit_spec(self, spec=None, joint_names=None) -> MotorActuatorGroup:
    return self._base_actuator.edit_spec(spec, joint_names)

  def initialize(self, mj_model, model, data, device: str) -> None:
    self._base_actuator._ctrl_ids_list = self._ctrl_ids_list
    self._base_actuator.initialize(mj_model, model, data, device)
    self._joint_ids = self._base_actuator._joint_ids
    self._ctrl_ids = self._base_actuator._ctrl_ids
    c = self.cfg
    for t in c.targets:
      self._delay_buffers[t] = DelayBuffer(
          min_lag=c.delay_min_lag, max_lag=c.delay_max_lag, batch_size=_num_worlds(data),
          device=device, hold_prob=c.delay_hold_prob, update_period=c.delay_update_period,
          per_env_phase=c.delay_per_env_phase)

  @staticmethod
  def _delayed(buf: DelayBuffer, value: torch.Tensor, mask: torch.Tensor | None,
               hold: torch.Tensor | None = None) -> torch.Tensor:
    """Append `value` and read it `lag` steps late.  Rows outside `mask` keep their history,
    lag and step count exactly and read their held frame; rows of `hold` keep the lag that
    `set_lags(..., hold=True)` gave them."""
    buf.append(value, mask)
    return buf.compute(mask, hold)

  def compute(self, cmd: ActuatorCmd, mask: torch.Tensor | None = None) -> torch.Tensor:
    """`mask` (`[num_envs]` bool): the rows this call steps.  The sync-free env's post-reset
    `write_data_to_sim` passes its reset mask, so only the reset envs take that extra frame."""
    vals = dict(position=cmd.position_target, velocity=cmd.velocity_target, effort=cmd.effort_target)
    for t, buf in self._delay_buffers.items():
      vals[t] = self._delayed(buf, vals[t], mask, self._hold)
    late = ActuatorCmd(position_target=vals["position"], velocity_target=vals["velocity"],
                       effort_target=vals["effort"], joint_pos=cmd.joint_pos, joint_vel=cmd.joint_vel)
    if mask is not None and getattr(self._base_actuator, "takes_mask", False):
      return self._base_actuator.compute(late, mask=mask)
    return self._base_actuator.compute(late)

  def reset(self, env_ids=None) -> None:
    if self._engine is not None:
      self._engine[0].reset_rows(self._engine[1], env_ids=env_ids)
    else:
      for buf in self._delay_buffers.values():
        buf.reset(env_ids)
      if self._hold is not None:
        self._hold[slice(None) if env_ids is None else env_ids] = False
    self._base_actuator.reset(env_ids)

  def reset_masked(self, mask: torch.Tensor) -> None:
    if self._engine is not None:
      self._engine[0].reset_rows(self._engine[1], mask=mask.bool())
    else:
      for buf in self._delay_buffers.values():
        buf.reset_masked(mask)
      if self._hold is not None:
        self._hold &= ~mask.bool()
    self._base_actuator.reset_masked(mask)

  def set_lags(self, lags: torch.Tensor, env_ids=None, hold: bool = False) -> None:
    """Lags in physics steps, scalar or `[len(env_ids)]`, clamped to the cfg's range; the
    next `compute` redraws them unless `delay_hold_prob` / `delay_update_period` hold.  With
    `hold` these rows keep the lag until their next reset (or a `set_lags` without it)."""
    if self._engine is not None:
      self._engine[0].set_lags(self._engine[1], lags, env_ids, hold)
      return
    for buf in self._delay_buffers.values():
      buf.set_lags(lags, env_ids)
    if hold or self._hold is not None:
      buf = next(iter(self._delay_buffers.values()))
      if self._hold is None:
        self._hold = torch.zeros(buf.batch_size, dtype=torch.bool, device=buf.current_lags.device)
      self._hold[slice(None) if env_ids is None else env_ids] = bool(hold)

  def update(self, dt: float) -> None:
    self._base_actuator.update(dt)


def engine_kind(act: Actuator) -> int | None:
  """The engine's kind of an explicit actuator, None where only torch evaluates it (the
  delay wrapper)."""
  return getattr(act, "engine_kind", None)


# ---------------------------------------------------------------------------------------------
# engine mode: the laws run in the step kernels' phase A (include/mjx355.h mjxActuatorDesc)

_VP = ctypes.c_void_p


class ActuatorDesc(ctypes.Structure):
  """`mjxActuatorDesc` (include/mjx355.h); `mjx_actuator_desc_size` guards the layout."""
  _fields_ = ([("nworld", ctypes.c_int32), ("nu", ctypes.c_int32), ("ring_len", ctypes.c_int32),
               ("reserved", ctypes.c_int32), ("kind", _VP), ("min_lag", _VP), ("max_lag", _VP),
               ("group", _VP), ("seed", ctypes.c_uint64)]
              + [(n, _VP) for n in ("kp", "kd", "effort_limit", "saturation_effort", "velocity_limit",
                                    "corner_velocity", "position_target", "velocity_target",
                                    "effort_target", "ring", "lag", "pushes", "draws", "hold")])


class ActuatorNet(ctypes.Structure):
  """`mjxActuatorNet` (include/mjx355.h)."""
  _fields_ = [("nlayer", ctypes.c_int32), ("history", ctypes.c_int32), ("input_order", ctypes.c_int32),
              ("reserved", ctypes.c_int32), ("width", ctypes.c_int32 * (MAX_NET_LAYERS + 1)),
              ("activation", ctypes.c_int32 * MAX_NET_LAYERS), ("pos_scale", ctypes.c_float),
              ("vel_scale", ctypes.c_float), ("torque_scale", ctypes.c_float),
              ("weight", _VP * MAX_NET_LAYERS), ("bias", _VP * MAX_NET_LAYERS)]


class ActuatorNetDesc(ctypes.Structure):
  """`mjxActuatorNetDesc` (include/mjx355.h); `mjx_actuator_net_desc_size` guards the layout."""
  _fields_ = [("nworld", ctypes.c_int32), ("nu", ctypes.c_int32), ("nnet", ctypes.c_int32),
              ("hist_len", ctypes.c_int32), ("nets", ActuatorNet * MAX_NETS), ("net", _VP),
              ("history", _VP), ("staging", _VP), ("pushes", _VP)]


NO_NET = 255
MAX_ENGINE_LAG = 32  # csrc/engine.h kMaxActLag


def engine_unsupported(act: Actuator) -> str | None:
  """Why the engine cannot run `act` (None: it can).  Engine mode covers the ideal-PD and DC
  laws and a learned actuator whose module is a plain MLP (`extract_mlp`), bare or behind a
  delay, and a delayed builtin position group; a delay acts on the position target with a lag
  drawn every substep."""
  base = act.base_actuator if isinstance(act, DelayedActuator) else act
  if engine_kind(base) is None:
    what = type(base.cfg).__name__ if isinstance(base, BuiltinActuator) else type(base).__name__
    return f"{what} has no engine form"
  if isinstance(base, LearnedMlpActuator):
    why = base.mlp[1]
    if why is not None:
      return f"LearnedMlpActuator network {base.cfg.network_file!r}: {why}"
  if isinstance(act, DelayedActuator):
    c = act.cfg
    if c.targets != ("position",):
      return f"delay_target {c.delay_target!r} (the engine delays the position target only)"
    if c.delay_hold_prob != 0.0 or c.delay_update_period != 0:
      return "delay_hold_prob / delay_update_period (the engine redraws the lag every substep)"
    if c.delay_max_lag > MAX_ENGINE_LAG:
      return f"delay_max_lag {c.delay_max_lag} > {MAX_ENGINE_LAG}"
  return None


class EngineActuators:
  """The explicit actuators of a simulation bound to the engine (`Simulation.
  set_explicit_actuators`).  Owns the `[num_envs, nu]` buffers the step kernels read; each
  actuator's gain / limit tensors become column views of them, so `set_gains`,
  `set_effort_limit` and `set_lags` act on the engine without a copy or another call.

  The delay state lives here in engine mode (`ring`, `lag`, `pushes`, `draws`; the torch
  `DelayBuffer`s rest): phase C pushes a frame per integrated substep, a reset clears a
  world's history and marks it, and the next `write_targets` primes the marked worlds with
  one frame of their target -- the frame the reference's post-reset `write_data_to_sim`
  appends."""

  def __init__(self, sim, entities, seed: int | None = None):
    m = sim.mj_model
    n, nu, dev = int(sim.num_envs), int(m.nu), sim._torch_device
    self.sim, self.entities = sim, list(entities)
    self._check_bindable(self.entities)  # every refusal, before any actuator's state is touched
    f = lambda v=0.0: torch.full((n, nu), float(v), dtype=torch.float32, device=dev)
    z32 = lambda: torch.zeros(n, nu, dtype=torch.int32, device=dev)
    self.kp, self.kd, self.effort_limit = f(), f(), f()
    self.saturation_effort, self.velocity_limit, self.corner_velocity = f(1.0), f(1.0), f()
    self.position_target, self.velocity_target, self.effort_target = f(), f(), f()
    self.lag, self.pushes, self.draws, self.hold = z32(), z32(), z32(), z32()
    self.prime = torch.zeros(n, nu, dtype=torch.bool, device=dev)
    kind, lo, hi, grp = ([0] * nu for _ in range(4))
    self._bound, group = [], 0
    net_of, hcap = [NO_NET] * nu, [0] * nu
    self._nets, self._net_keys, self._learned = [], {}, []  # (spec, cfg), key -> index, (act, sl, ent)
    for ent in self.entities:
      acts = ent.custom_actuators
      gid = ent.indexing.ctrl_ids.tolist()
      explicit_local = set()
      for act in acts:
        why = engine_unsupported(act)
        if why is not None:
          raise ValueError(f"entity '{ent.name}': {why}")
        base = act.base_actuator if isinstance(act, DelayedActuator) else act
        cols = [gid[c] for c in act._ctrl_ids_list]
        if cols != list(range(cols[0], cols[0] + len(cols))):
          raise ValueError(f"entity '{ent.name}': the actuators of {act.joint_names} are not "
                           "contiguous in the model")
        sl = slice(cols[0], cols[0] + len(cols))
        pairs = []
        if isinstance(base, IdealPdActuator):
          pairs = [("stiffness", self.kp), ("damping", self.kd), ("force_limit", self.effort_limit)]
        if isinstance(base, DcMotorActuator):
          pairs += [("saturation_effort", self.saturation_effort),
                    ("velocity_limit_motor", self.velocity_limit),
                    ("_vel_at_effort_lim", self.corner_velocity)]
        for name, buf in pairs:
          buf[:, sl] = getattr(base, name)
          setattr(base, name, buf[:, sl])
        delayed = isinstance(act, DelayedActuator)
        for c in cols:
          kind[c], grp[c] = engine_kind(base), group
          if delayed:
            lo[c], hi[c] = int(act.cfg.delay_min_lag), int(act.cfg.delay_max_lag)
        if delayed:
          act._engine = (self, sl)
        if isinstance(base, LearnedMlpActuator):
          spec, c = base.mlp[0], base.cfg
          key = self._net_key(base)
          if key not in self._net_keys:
            self._net_keys[key] = len(self._nets)
            self._nets.append((spec, c))
          for col in cols:
            net_of[col], hcap[col] = self._net_keys[key], c.history_length - 1
          self._learned.append((base, sl, ent))
        self._bound.append((act, sl))
        explicit_local.update(act._ctrl_ids_list)
        group += 1
      if not acts:
        continue
      t = lambda x: torch.as_tensor(x, dtype=torch.long, device=dev)
      loc = sorted(explicit_local)
      rest = [c for c in range(len(gid)) if c not in explicit_local]
      ent._engine_cols = (t([gid[c] for c in loc]), t([ent._act_joint_local[c] for c in loc]),
                          t([gid[c] for c in rest]), t([ent._act_joint_local[c] for c in rest]))
    if not self._bound:
      raise ValueError("set_explicit_actuators: no explicit actuator among the entities")
    self.ring_len = max(hi)
    self.ring = (torch.zeros(n, self.ring_len, nu, dtype=torch.float32, device=dev)
                 if self.ring_len > 0 else None)
    self._lo_host, self._hi_host = lo, hi  # set_lags clamps without reading the device
    self._lo = torch.tensor(lo, dtype=torch.int32, device=dev)
    self._delayed = torch.tensor([h > 0 for h in hi], dtype=torch.bool, device=dev)
    self._span = torch.tensor([h - l + 1 for l, h in zip(lo, hi)], dtype=torch.int32, device=dev)
    self._group = torch.tensor(grp, dtype=torch.long, device=dev)
    self.lag.copy_(self._fresh_lags())
    for act, sl in self._bound:  # continue from the history the torch path holds
      if isinstance(act, DelayedActuator) and self.ring is not None:
        self._take_over(act._delay_buffers["position"], sl)
    self.seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else int(seed)
    u8 = lambda v: (ctypes.c_uint8 * nu)(*v)
    self._tables = [u8(kind), u8(lo), u8(hi), u8(grp)]
    d = ActuatorDesc()
    d.nworld, d.nu, d.ring_len, d.seed = n, nu, self.ring_len, self.seed
    d.kind, d.min_lag, d.max_lag, d.group = (ctypes.cast(t, _VP) for t in self._tables)
    for name in ("kp", "kd", "effort_limit", "saturation_effort", "velocity_limit",
                 "corner_velocity", "position_target", "velocity_target", "effort_target", "lag",
                 "pushes", "draws", "hold"):
      setattr(d, name, getattr(self, name).data_ptr())
    d.ring = self.ring.data_ptr() if self.ring is not None else None
    self.desc = d
    self._bind_nets(net_of, hcap)
    for ent in self.entities:
      if ent.custom_actuators:
        ent._engine_actuators = self

  # ---------------------------------------------------------------- learned actuators
  def _bind_nets(self, net_of, hcap) -> None:
    """The network descriptor (`mjxActuatorNetDesc`) and the history the engine keeps for the
    learned actuators: `hist` `[num_envs, hist_len, 2, nu]` (hist_len = the largest
    history_length - 1; oldest frame first; position error, then velocity), the frame phase A
    staged (`stage`) and the frames pushed since the reset (`hpush`, at most history_length - 1
    per actuator).  A reset clears a world's rows and marks them (`net_prime`); the next
    `write_targets` primes them with the frame the torch path's post-reset
    `write_data_to_sim` appends."""
    self.net_desc = None
    self.hist = self.stage = self.hpush = None
    if not self._nets:
      return
    n, nu = self.lag.shape
    dev = self.lag.device
    self.hist_len = max(hcap)
    self.hpush = torch.zeros(n, nu, dtype=torch.int32, device=dev)
    self.stage = torch.zeros(n, 2, nu, dtype=torch.float32, device=dev)
    self.net_prime = torch.zeros(n, nu, dtype=torch.bool, device=dev)
    self._is_learned = torch.tensor([k != NO_NET for k in net_of], dtype=torch.bool, device=dev)
    self._first_push = torch.tensor([min(h, 1) for h in hcap], dtype=torch.int32, device=dev)
    self._jp = torch.zeros(n, nu, dtype=torch.float32, device=dev)  # reset_masked's joint state
    self._jv = torch.zeros(n, nu, dtype=torch.float32, device=dev)
    if self.hist_len > 0:
      self.hist = torch.zeros(n, self.hist_len, 2, nu, dtype=torch.float32, device=dev)
    t = lambda x: torch.as_tensor(x, dtype=torch.long, device=dev)
    self._net_cols = {}
    for ent in self.entities:
      gid = ent.indexing.ctrl_ids.tolist()
      loc = sorted(c for base, _, e in self._learned if e is ent for c in base._ctrl_ids_list)
      if loc:
        self._net_cols[id(ent)] = (ent, t([gid[c] for c in loc]), t([ent._act_joint_local[c] for c in loc]))
    for base, sl, _ in self._learned:  # continue from the history the torch path holds
      self._take_over_net(base, sl)
      base._engine = (self, sl)
    d = ActuatorNetDesc()
    d.nworld, d.nu, d.nnet, d.hist_len = n, nu, len(self._nets), self.hist_len
    self._net_keep = [(ctypes.c_uint8 * nu)(*net_of)]
    d.net = ctypes.cast(self._net_keep[0], _VP)
    for k, (spec, c) in enumerate(self._nets):
      e = d.nets[k]
      e.nlayer, e.history = len(spec.weights), c.history_length
      e.input_order = _INPUT_ORDERS.index(c.input_order)
      e.pos_scale, e.vel_scale, e.torque_scale = c.pos_scale, c.vel_scale, c.torque_scale
      for l, w in enumerate(spec.widths):
        e.width[l] = w
      for l, (w, b) in enumerate(zip(spec.weights, spec.biases)):
        e.activation[l] = spec.activations[l]
        e.weight[l], e.bias[l] = w.data_ptr(), b.data_ptr()
        self._net_keep += [w, b]
    if self.hist is not None:
      d.history, d.staging, d.pushes = self.hist.data_ptr(), self.stage.data_ptr(), self.hpush.data_ptr()
    self.net_desc = d

  def _net_frames(self, base, sl):
    """The engine's columns of the `history_length - 1` frames before the current one, and the
    torch buffers that hold them after the frame of their last `compute`."""
    h = base.cfg.history_length - 1
    mine = self.hist[:, self.hist_len - h:, :, sl]
    return h, mine, base._pos_error_history, base._vel_history

  def _take_over_net(self, base, sl) -> None:
    if base.cfg.history_length < 2 or not base._pos_error_history.is_initialized:
      return  # no history, or nothing appended yet: the engine starts empty as well
    h, mine, pos, vel = self._net_frames(base, sl)
    mine[:, :, 0] = pos.buffer[:, 1:]
    mine[:, :, 1] = vel.buffer[:, 1:]
    self.hpush[:, sl] = pos.num_pushes.clamp(max=h).to(torch.int32).unsqueeze(1)

  def _hand_back_net(self, base, sl) -> None:
    if base.cfg.history_length < 2:
      return
    h, mine, pos, vel = self._net_frames(base, sl)
    for k, buf in enumerate((pos, vel)):
      if not buf.is_initialized:
        buf.append(torch.zeros_like(self.position_target[:, sl]))  # allocates the frames
      buf.buffer[:, 1:] = mine[:, :, k]
      buf.buffer[:, 0] = buf.buffer[:, 1]  # (the next append drops it)
      buf.num_pushes.copy_(self.hpush[:, sl.start])

  def reset_net_rows(self, sl: slice, env_ids=None, mask: torch.Tensor | None = None) -> None:
    if self.hist is None:
      return
    if mask is None:
      mask = torch.zeros(self.lag.shape[0], dtype=torch.bool, device=self.lag.device)
      mask[slice(None) if env_ids is None else env_ids] = True
    m = mask.view(-1, 1)
    self.hpush[:, sl] = torch.where(m, torch.zeros_like(self.hpush[:, sl]), self.hpush[:, sl])
    self.hist[:, :, :, sl] = torch.where(m.view(-1, 1, 1, 1), torch.zeros_like(self.hist[:, :, :, sl]),
                                         self.hist[:, :, :, sl])
    self.net_prime[:, sl] |= m

  def _prime_nets(self, ent) -> None:
    """The marked rows of `ent`'s learned actuators take one frame of their post-reset target
    and joint state (fixed ops: graph-capturable)."""
    if self.hist is None or id(ent) not in self._net_cols:
      return
    _, gc, jl = self._net_cols[id(ent)]
    d = ent.data
    p = self.net_prime[:, gc]
    newest = self.hist[:, -1]
    newest[:, 0, gc] = torch.where(p, self.position_target[:, gc] - d.joint_pos[:, jl], newest[:, 0, gc])
    newest[:, 1, gc] = torch.where(p, d.joint_vel[:, jl], newest[:, 1, gc])
    self.hpush[:, gc] = torch.where(p, self._first_push[gc].expand_as(p), self.hpush[:, gc])
    self.net_prime.index_fill_(1, gc, False)

  def _reset_nets_masked(self, mask: torch.Tensor) -> None:
    """`reset_net_rows` and `_prime_nets` in one for a fused env step: whole buffers, fixed ops."""
    if self.hist is None:
      return
    for ent, gc, jl in self._net_cols.values():
      self._jp[:, gc] = ent.data.joint_pos[:, jl]
      self._jv[:, gc] = ent.data.joint_vel[:, jl]
    m = mask.bool().view(-1, 1) & self._is_learned
    self.hpush.copy_(torch.where(m, self._first_push.expand_as(m), self.hpush))
    self.hist.masked_fill_(m.view(m.shape[0], 1, 1, -1), 0.0)
    newest = self.hist[:, -1]
    newest[:, 0].copy_(torch.where(m, self.position_target - self._jp, newest[:, 0]))
    newest[:, 1].copy_(torch.where(m, self._jv, newest[:, 1]))
    self.net_prime.masked_fill_(m, False)

  @staticmethod
  def _net_key(base):
    """Equal for learned actuators that share one engine network: the same layers, history,
    input order and scales (the scales are the network's in the engine's descriptor)."""
    c = base.cfg
    return (base.mlp[0].key(), c.history_length, c.input_order, float(c.pos_scale), float(c.vel_scale),
            float(c.torque_scale))

  @classmethod
  def _check_bindable(cls, entities) -> None:
    """ValueError for what the engine cannot bind, raised while nothing is bound yet: the
    constructor below rebinds the actuators' tensors and routes their resets to itself as it
    goes, and a refusal half-way would leave them pointing at a dead binding."""
    keys, any_act = set(), False
    for ent in entities:
      gid = ent.indexing.ctrl_ids.tolist()
      for act in ent.custom_actuators:
        any_act = True
        why = engine_unsupported(act)
        if why is not None:
          raise ValueError(f"entity '{ent.name}': {why}")
        cols = [gid[c] for c in act._ctrl_ids_list]
        if cols != list(range(cols[0], cols[0] + len(cols))):
          raise ValueError(f"entity '{ent.name}': the actuators of {act.joint_names} are not "
                           "contiguous in the model")
        base = act.base_actuator if isinstance(act, DelayedActuator) else act
        if isinstance(base, LearnedMlpActuator):
          keys.add(cls._net_key(base))
          if len(keys) > MAX_NETS:
            raise ValueError(
                f"entity '{ent.name}': more than {MAX_NETS} different actuator networks (a network "
                "is its layers with its history_length, input_order and the three scales)")
    if not any_act:
      raise ValueError("set_explicit_actuators: no explicit actuator among the entities")

  def _fresh_lags(self) -> torch.Tensor:
    """`[num_envs, nu]` int32 lags as after a reset: uniform on each group's range, one draw
    per world and group (a fixed range gives its one value)."""
    n, nu = self.lag.shape
    u = torch.rand(n, nu, device=self.lag.device)[:, self._group]  # a group's columns share
    return (self._lo + (u * self._span).floor().to(torch.int32).clamp_max(self._span - 1))

  def _frames(self, buf: DelayBuffer, sl: slice):
    """The `k` newest frames the two rings share: the torch ring's (`[n, max_lag + 1, nj]`,
    oldest first, the newest being the last target appended) and the engine's columns."""
    ring = buf._buffer
    k = min(ring.max_length, self.ring_len)
    return ring, ring.max_length - k, self.ring[:, self.ring_len - k:, sl]

  def _take_over(self, buf: DelayBuffer, sl: slice) -> None:
    if not buf.is_initialized:
      return  # nothing appended yet: the engine starts empty as well
    ring, at, mine = self._frames(buf, sl)
    mine.copy_(ring.buffer[:, at:])
    self.pushes[:, sl] = ring.num_pushes.clamp(max=self.ring_len).to(torch.int32).unsqueeze(1)
    # (the lag is not carried: either path draws the lag of its next read anew)

  def _hand_back(self, buf: DelayBuffer, sl: slice) -> None:
    if not buf.is_initialized:
      buf.append(self.position_target[:, sl])  # allocates the frames; overwritten below
    ring, at, mine = self._frames(buf, sl)
    ring.buffer[:, at:] = mine
    ring.num_pushes.copy_(self.pushes[:, sl.start])

  def release(self) -> None:
    """The delay history goes back to the actuators' torch buffers."""
    for ent in self.entities:
      ent._engine_actuators = None
    for act, sl in self._bound:
      if isinstance(act, DelayedActuator):
        if self.ring is not None:
          self._hand_back(act._delay_buffers["position"], sl)
        act._engine = None
    for base, sl, _ in self._learned:  # ... and the network history to the learned actuators'
      if self.hist is not None:
        self._hand_back_net(base, sl)
      base._engine = None

  # ---------------------------------------------------------------- per step
  def write_targets(self, ent) -> None:
    """`Entity.write_data_to_sim` in engine mode: the builtin actuators' ctrl as before, the
    explicit actuators' three targets into the engine's buffers, and the post-reset frame of
    the worlds a reset marked.  Fixed tensor ops: no host sync, graph-capturable."""
    gc, jl, gb, jb = ent._engine_cols
    d = ent.data
    if gb.numel():
      d.data.ctrl[:, gb] = d.joint_pos_target[:, jb]
    self.position_target[:, gc] = d.joint_pos_target[:, jl]
    self.velocity_target[:, gc] = d.joint_vel_target[:, jl]
    self.effort_target[:, gc] = d.joint_effort_target[:, jl]
    if self.ring is not None:
      p = self.prime[:, gc]
      newest = self.ring[:, -1]
      newest[:, gc] = torch.where(p, self.position_target[:, gc], newest[:, gc])
      self.pushes[:, gc] = torch.where(p, torch.ones_like(self.pushes[:, gc]), self.pushes[:, gc])
      self.prime.index_fill_(1, gc, False)  # (a kernel argument: records into a graph)
    self._prime_nets(ent)

  # ---------------------------------------------------------------- delay state (per group)
  def reset_rows(self, sl: slice, env_ids=None, mask: torch.Tensor | None = None) -> None:
    if self.ring is None:  # every lag range is [0, 0]: there is no history to clear
      return
    if mask is None:
      mask = torch.zeros(self.lag.shape[0], dtype=torch.bool, device=self.lag.device)
      mask[slice(None) if env_ids is None else env_ids] = True
    m = mask.view(-1, 1)
    self.pushes[:, sl] = torch.where(m, torch.zeros_like(self.pushes[:, sl]), self.pushes[:, sl])
    self.lag[:, sl] = torch.where(m, self._fresh_lags()[:, sl], self.lag[:, sl])
    self.hold[:, sl] = torch.where(m, torch.zeros_like(self.hold[:, sl]), self.hold[:, sl])
    self.ring[:, :, sl] = torch.where(m.unsqueeze(1), torch.zeros_like(self.ring[:, :, sl]),
                                      self.ring[:, :, sl])
    self.prime[:, sl] |= m

  def reset_masked(self, mask: torch.Tensor) -> None:
    """A fused env step's reset of the worlds in `mask`, after the task's reset kernel has
    cleared their targets: every delayed actuator's history cleared and primed with one frame
    of the post-reset target (`reset_rows` and the priming of `write_targets` in one, whole
    buffers and fixed ops: records into a HIP graph)."""
    self._reset_nets_masked(mask)
    if self.ring is None:
      return
    m = mask.bool().view(-1, 1) & self._delayed
    self.pushes.copy_(torch.where(m, torch.ones_like(self.pushes), self.pushes))
    self.lag.copy_(torch.where(m, self._fresh_lags(), self.lag))
    self.hold.masked_fill_(m, 0)
    self.ring.masked_fill_(m.unsqueeze(1), 0.0)
    newest = self.ring[:, -1]
    newest.copy_(torch.where(m, self.position_target, newest))
    self.prime.masked_fill_(m, False)

  def set_lags(self, sl: slice, lags: torch.Tensor, env_ids=None, hold: bool = False) -> None:
    """`hold`: phase C's push draws no new lag for these rows until their reset."""
    rows = slice(None) if env_ids is None else env_ids
    lo, hi = self._lo_host[sl.start], self._hi_host[sl.start]
    lags = torch.as_tensor(lags, device=self.lag.device).clamp(lo, hi).to(torch.int32)
    self.lag[rows, sl] = lags.unsqueeze(-1) if lags.ndim == 1 else lags
    self.hold[rows, sl] = int(bool(hold))
