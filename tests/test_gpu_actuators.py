"""Explicit actuators on the GPU: the torch path (mjlab_amd/actuator.py) and the engine's
phase-A form (mjx_sim_set_actuators, csrc/engine_impl.h explicit_ctrl / act_push).

Scenes are the Go1 and G1 flat velocity scenes with every builtin position group replaced by
an IdealPdActuatorCfg / DcMotorActuatorCfg / DelayedActuatorCfg at the asset's own gains.
Worlds are seeded perturbations of the keyframe; the position targets are the joint positions
plus an error drawn on +-2 effort_limit / kp, so the effort clamp binds for about half of
the actuators and not for the rest (both populations are asserted).

Engine mode and torch mode run the same individually rounded operations in the same order,
so `step(4)` in engine mode and four rounds of `write_data_to_sim()` + `step(1)` in torch
mode are compared bit for bit (every parity_util.DATA_FIELDS field and ctrl), like the
project's fused-vs-single step tests.

Faults: a test that meets a HIP illegal access or launch failure sets a module flag and every later test fails at
once without touching the GPU (the rule of tests/test_gpu_kernel_variants.py)."""

from __future__ import annotations

import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

from parity_util import DATA_FIELDS, g1_states

pytestmark = pytest.mark.gpu

GO1, G1 = "Mjlab-Velocity-Flat-Unitree-Go1", "Mjlab-Velocity-Flat-Unitree-G1"
U = 2.0 ** -24  # fp32 unit roundoff
FIELDS = DATA_FIELDS + ("ctrl",)
_faulted = []


def guarded(fn):
  @functools.wraps(fn)
  def run(*a, **k):
    if _faulted:
      pytest.fail(f"not run: an earlier test met a GPU fault ({_faulted[0]})")
    try:
      return fn(*a, **k)
    except Exception as e:  # noqa: BLE001
      if "illegal memory access" in str(e) or "unspecified launch failure" in str(e):
        _faulted.append(f"{fn.__name__}: {str(e)[:200]}")
      raise
  return run


# ------------------------------------------------------------------ scenes
def _pd(g):
  from mjlab_amd.actuator import IdealPdActuatorCfg
  return IdealPdActuatorCfg(joint_names_expr=g.joint_names_expr, stiffness=g.stiffness,
                            damping=g.damping, effort_limit=g.effort_limit, armature=g.armature)


DC_SAT, DC_VLIM = 1.5, 10.0  # stall torque over the rating; no-load speed, rad/s


def _dc(g):
  from mjlab_amd.actuator import DcMotorActuatorCfg
  return DcMotorActuatorCfg(joint_names_expr=g.joint_names_expr, stiffness=g.stiffness,
                            damping=g.damping, effort_limit=g.effort_limit, armature=g.armature,
                            saturation_effort=DC_SAT * g.effort_limit, velocity_limit=DC_VLIM)


def _delayed(lo, hi, base=_pd, **kw):
  def make(g):
    from mjlab_amd.actuator import DelayedActuatorCfg
    return DelayedActuatorCfg(base_cfg=base(g), delay_min_lag=lo, delay_max_lag=hi, **kw)
  return make


class Rig:
  """A scene + Simulation without the env managers."""

  def __init__(self, task, make, n, device, capacity=None, engine=False, seed=5):
    from mjlab_amd.envs import load_env_cfg
    from mjlab_amd.scene import Scene
    from mjlab_amd.sim import Simulation
    cfg = load_env_cfg(task)
    cfg.scene.num_envs = n
    art = cfg.scene.entities["robot"].articulation
    self.groups = tuple(art.actuators)
    if make is not None:
      art.actuators = tuple(make(g) for g in art.actuators)
    if capacity is not None:
      cfg.sim.engine_capacity = capacity
      cfg.sim.specialize = "never"
    self.scene = Scene(cfg.scene, device)
    model = self.scene.compile()
    with warnings.catch_warnings():
      warnings.simplefilter("ignore")  # (the small carve has no specialised kernels)
      self.sim = Simulation(n, cfg.sim, model, device)
    self.scene.initialize(self.sim.mj_model, self.sim.model, self.sim.data)
    self.robot = self.scene["robot"]
    self.n, self.device, self.model = n, device, model
    self.engine = self.sim.set_explicit_actuators(self.scene.entities.values(), seed=seed) if engine else None

  def gains(self):
    """Per actuator (entity order): kp, kd, effort limit, as numpy float32."""
    kp, kd, lim = (np.zeros(len(self.robot.actuator_names), np.float32) for _ in range(3))
    import re
    for g in self.groups:
      for i, name in enumerate(self.robot.actuator_names):
        if any(re.fullmatch(e, name) for e in g.joint_names_expr):
          kp[i], kd[i], lim[i] = g.stiffness, g.damping, g.effort_limit
    return kp, kd, lim

  def load(self, q, qv):
    """A reset of every world, as the env's reset(): state, cleared actuators, then the
    post-reset write and forward."""
    t = lambda x: torch.as_tensor(x, dtype=torch.float32, device=self.device)
    self.sim.reset()
    self.scene.reset()
    self.sim.data.qpos[:] = t(q)
    self.sim.data.qvel[:] = t(qv)
    self.scene.write_data_to_sim()
    self.sim.forward()

  def target(self, tgt):
    self.robot.set_joint_position_target(torch.as_tensor(tgt, dtype=torch.float32, device=self.device))

  def env_step(self, nsub=4):
    if self.engine is not None:
      self.scene.write_data_to_sim()
      self.sim.step(nsub)
    else:
      for _ in range(nsub):
        self.scene.write_data_to_sim()
        self.sim.step(1)

  def fields(self):
    return {k: getattr(self.sim.data, k).clone() for k in FIELDS}


def _states(rig, seed, vel_scale=0.5):
  q, qv, _ = g1_states(rig.model, rig.n, seed=seed, vel_scale=vel_scale)
  return q, qv


def _joint_q(rig, q):
  return np.asarray(q)[:, rig.robot.indexing.joint_q_adr.cpu().numpy()][:, rig.robot._act_joint_local]


def _joint_v(rig, qv):
  return np.asarray(qv)[:, rig.robot.indexing.joint_v_adr.cpu().numpy()][:, rig.robot._act_joint_local]


def _targets(rig, q, seed):
  """Joint-order targets: the joint position plus an error on +-2 effort_limit / kp."""
  kp, _, lim = rig.gains()
  rng = np.random.default_rng(seed)
  err = rng.uniform(-2.0, 2.0, (rig.n, len(kp))) * (lim / kp)
  tgt_act = _joint_q(rig, q) + err
  tgt = np.zeros((rig.n, rig.robot.num_joints))
  tgt[:, rig.robot._act_joint_local] = tgt_act
  return tgt.astype(np.float32), tgt_act.astype(np.float32)


def _assert_equal(a, b, what, rows=None):
  for k in FIELDS:
    x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
    if not torch.equal(x, y):
      bad = (x != y).reshape(x.shape[0], -1).any(dim=1).nonzero().flatten().tolist()
      d = (x.double() - y.double()).abs().max().item()
      pytest.fail(f"{what}: {k} differs in {len(bad)} worlds (first {bad[:5]}), max |diff| {d:.3e}")


# ------------------------------------------------------------------ 1. ideal PD = builtin position
@pytest.mark.parametrize("task,n", [(GO1, 64), (G1, 96)])
@guarded
def test_ideal_pd_matches_builtin_position(task, n, gpu_device):
  """actuator_force after forward at the same state and target: the builtin position actuator
  (kp c - kp q - kd qd, each product and sum rounded) against the ideal-PD <motor> (kp (c - q)
  + kd (0 - qd)), torch and engine mode.  Bound per actuator, first order in the fp32 unit
  roundoff u = 2^-24: the explicit form rounds c - q, two products and two sums, each error
  at most u times kp |c - q| or kd |qd|; the builtin form rounds three products and two sums
  of terms kp |c|, kp |q|, kd |qd|.  Every term is counted four times (more roundings than
  either form has, which also covers the second-order terms); the force clamp is 1-Lipschitz."""
  builtin = Rig(task, None, n, gpu_device)
  torch_pd = Rig(task, _pd, n, gpu_device)
  engine_pd = Rig(task, _pd, n, gpu_device, engine=True)
  q, qv = _states(builtin, seed=11)
  tgt, tgt_act = _targets(builtin, q, seed=12)
  kp, kd, lim = builtin.gains()
  for r in (builtin, torch_pd, engine_pd):
    r.load(q, qv)
    r.target(tgt)
    r.scene.write_data_to_sim()
    r.sim.forward()
  ref = builtin.sim.data.actuator_force.cpu().numpy()
  qa, va = _joint_q(builtin, q).astype(np.float32), _joint_v(builtin, qv).astype(np.float32)
  bound = 4 * U * (kp * np.abs(tgt_act - qa) + kp * np.abs(tgt_act) + kp * np.abs(qa) + 2 * kd * np.abs(va))
  clamped = np.abs(ref) == lim
  assert clamped.any(axis=1).sum() > 0 and (~clamped).sum() > 0 and clamped.sum() > 0
  assert (~clamped.any(axis=1)).sum() + (clamped.all(axis=1)).sum() < n  # worlds with both kinds
  for name, r in (("torch", torch_pd), ("engine", engine_pd)):
    got = r.sim.data.actuator_force.cpu().numpy()
    err = np.abs(got - ref)
    print(f"{task} {name}: max |diff| {err.max():.3e}, max diff / bound {np.max(err / bound):.3f}")
    assert (err <= bound).all(), f"{name}: {np.argwhere(err > bound)[:5]}"
  # the two explicit forms are the same operations: equal bits, and ctrl shows the torque
  assert torch.equal(torch_pd.sim.data.actuator_force, engine_pd.sim.data.actuator_force)
  assert torch.equal(torch_pd.sim.data.ctrl, engine_pd.sim.data.ctrl)
  assert torch.equal(engine_pd.sim.data.ctrl, engine_pd.sim.data.actuator_force)


# ------------------------------------------------------------------ 2. engine = torch, bit for bit
def _twin_run(task, make, n, device, steps=6, capacity=None, graph=False, dc_vel=False):
  a = Rig(task, make, n, device, capacity=capacity, engine=True)
  b = Rig(task, make, n, device, capacity=capacity)
  q, qv = _states(a, seed=21, vel_scale=4.0 if dc_vel else 0.5)
  for r in (a, b):
    r.load(q, qv)
  g = None
  if graph:
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
      a.env_step()  # warm the launch path outside capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
      a.env_step()
    a.load(q, qv)
  for step in range(steps):
    tgt, _ = _targets(a, q, seed=100 + step)  # new targets every env step
    for r in (a, b):
      r.target(tgt)
    if g is not None:
      g.replay()
    else:
      a.env_step()
    b.env_step()
    _assert_equal(a.fields(), b.fields(), f"env step {step}")
  return a, b


@pytest.mark.parametrize("task,n", [(GO1, 64), (G1, 96)])
@guarded
def test_engine_equals_torch_ideal_pd(task, n, gpu_device):
  a, _ = _twin_run(task, _pd, n, gpu_device)
  kp, kd, lim = a.gains()
  c = a.sim.data.ctrl.abs().cpu().numpy()
  assert (c == lim).any() and (c < lim).any()


@pytest.mark.parametrize("lag", [0, 1, 2, 5])
@guarded
def test_engine_equals_torch_fixed_lag(lag, gpu_device):
  """Lags 0, 1, 2 and 5 substeps (5 > the 4 substeps of an env step: the delayed frame comes
  from the env step before, so the ring is read across the env-step boundary)."""
  _twin_run(GO1, _delayed(lag, lag), 64, gpu_device)


@guarded
def test_engine_equals_torch_delayed_g1(gpu_device):
  _twin_run(G1, _delayed(3, 3), 96, gpu_device)


@guarded
def test_engine_equals_torch_graph(gpu_device):
  """The engine-mode env step (targets + step(4)) captured in a HIP graph and replayed."""
  _twin_run(GO1, _delayed(2, 2), 64, gpu_device, graph=True)


@guarded
def test_engine_equals_torch_small_carve(gpu_device):
  """At a 20-contact / 80-row fast carve some worlds overflow and are re-solved in the max
  carve: their phase A runs twice in the substep, the delay ring is pushed once."""
  a, _ = _twin_run(G1, _delayed(2, 2), 96, gpu_device, capacity=(20, 80))
  assert a.sim.stats()["resolved"] > 0


# ------------------------------------------------------------------ 3. DC motor
def _dc_reference(rig, tgt_act, qa, va):
  """The law in float64 at fp32 inputs, and its rounding bound: six roundings of terms up to
  P = kp |pt - q| + kd |qd| on the PD side, three (quotient, difference, product) of terms up
  to S = saturation_effort (1 + |v| / velocity_limit) on the torque-speed side; the clamps
  are 1-Lipschitz in every argument."""
  e = rig.engine  # the engine's own fp32 parameters (one entity: its columns are the actuators)
  kp, kd, lim, sat, vlim, vc = (getattr(e, k)[0].double().cpu().numpy() for k in (
      "kp", "kd", "effort_limit", "saturation_effort", "velocity_limit", "corner_velocity"))
  assert np.allclose(vc, vlim * (1 + lim / sat), rtol=1e-6) and np.allclose(sat, DC_SAT * lim, rtol=1e-6)
  pt, qa, va = (x.astype(np.float64) for x in (tgt_act, qa, va))
  t = kp * (pt - qa) + kd * (0.0 - va)
  v = np.clip(va, -vc, vc)
  hi = np.minimum(sat * (1.0 - v / vlim), lim)
  lo = np.maximum(sat * (-1.0 - v / vlim), -lim)
  P = kp * np.abs(pt - qa) + kd * np.abs(va)
  S = sat * (1.0 + np.abs(v) / vlim)
  return np.minimum(np.maximum(t, lo), hi), U * (6 * P + 3 * S), (hi < lim) | (lo > -lim)


@guarded
def test_dc_motor_engine(gpu_device):
  n = 64
  a = Rig(GO1, _dc, n, gpu_device, engine=True)
  b = Rig(GO1, _dc, n, gpu_device)
  q, qv = _states(a, seed=31, vel_scale=4.0)
  tgt, tgt_act = _targets(a, q, seed=32)
  for r in (a, b):
    r.load(q, qv)
    r.target(tgt)
    r.scene.write_data_to_sim()
    r.sim.forward()

  def check(stage):
    qa = a.robot.data.joint_pos[:, a.robot._act_joint_local_t].cpu().numpy()
    va = a.robot.data.joint_vel[:, a.robot._act_joint_local_t].cpu().numpy()
    want, bound, speed_bound = _dc_reference(a, tgt_act, qa, va)
    got = a.sim.data.actuator_force.double().cpu().numpy()
    err = np.abs(got - want)
    print(f"dc {stage}: max |diff| {err.max():.3e}, max diff / bound {np.max(err / bound):.3f}, "
          f"torque-speed line binds for {speed_bound.mean():.2f} of the actuators")
    assert (err <= bound).all(), np.argwhere(err > bound)[:5]
    return speed_bound

  sb = check("forward")
  assert sb.any() and (~sb).any()
  _assert_equal(a.fields(), b.fields(), "dc forward")
  # a forward after step(4) evaluates the law at the stepped state (what the step's last
  # substep applied belongs to the state before its integration)
  a.env_step()
  b.env_step()
  _assert_equal(a.fields(), b.fields(), "dc step(4)")
  for r in (a, b):
    r.scene.write_data_to_sim()
    r.sim.forward()
  check("step(4) + forward")
  _assert_equal(a.fields(), b.fields(), "dc step(4) + forward")


# ------------------------------------------------------------------ 4. reset
@guarded
def test_masked_reset(gpu_device):
  n = 64
  make = _delayed(3, 3)
  a = Rig(GO1, make, n, gpu_device, engine=True)
  b = Rig(GO1, make, n, gpu_device)
  twin = Rig(GO1, make, n, gpu_device, engine=True)  # sees no reset
  q, qv = _states(a, seed=41)
  rigs = (a, b, twin)
  for r in rigs:
    r.load(q, qv)
  for step in range(2):
    tgt, _ = _targets(a, q, seed=200 + step)
    for r in rigs:
      r.target(tgt)
      r.env_step()
  mask = torch.zeros(n, dtype=torch.bool, device=gpu_device)
  mask[::2] = True
  ids = mask.nonzero().flatten()
  q2, qv2 = _states(a, seed=42)
  t = lambda x: torch.as_tensor(x, dtype=torch.float32, device=gpu_device)
  for r, masked in ((a, True), (b, False)):
    if masked:
      r.sim.reset_masked(mask)
      r.scene.reset_masked(mask)
    else:
      r.sim.reset(ids)
      r.scene.reset(ids)
    d = r.sim.data
    d.qpos[:] = torch.where(mask[:, None], t(q2), d.qpos)
    d.qvel[:] = torch.where(mask[:, None], t(qv2), d.qvel)
    r.scene.write_data_to_sim(mask=mask)
    r.sim.forward(mask)
  assert a.engine.pushes[ids].eq(1).all() and a.engine.pushes[~mask].eq(3).all()
  _assert_equal(a.fields(), b.fields(), "after the masked reset")
  for step in range(2):
    tgt, _ = _targets(a, q, seed=300 + step)
    for r in rigs:
      r.target(tgt)
      r.env_step()
    _assert_equal(a.fields(), b.fields(), f"reset twins, env step {step}")
    _assert_equal(a.fields(), twin.fields(), f"unreset worlds, env step {step}", rows=~mask)


# ------------------------------------------------------------------ 5. random lags
@guarded
def test_random_lags(gpu_device):
  """Lags drawn on [0, 3] by the engine's counter hash: 4,096 worlds, 200 substeps.  The
  pooled histogram of the 819,200 draws of the first group is tested against uniform with
  Pearson's chi-square, 3 degrees of freedom, at 30.66: the 1 - 1e-6 quantile, so a correct
  generator fails once in a million seeds (the seed here is fixed)."""
  n, steps = 4096, 200
  r = Rig(GO1, _delayed(0, 3), n, gpu_device, engine=True, seed=1234)
  q, qv = _states(r, seed=51)
  r.load(q, qv)
  tgt, _ = _targets(r, q, seed=52)
  r.target(tgt)
  eng = r.engine
  cols = [sl.start for _, sl in eng._bound]
  assert len(cols) == 2  # Go1: hips + thighs, calves

  def run(k):
    lags, pushes = [], []
    for _ in range(k):
      r.scene.write_data_to_sim()
      r.sim.step(1)
      lags.append(eng.lag[:, cols].clone())
      pushes.append(eng.pushes[:, cols[0]].clone())
    return torch.stack(lags).cpu().numpy(), torch.stack(pushes).cpu().numpy()

  lags, pushes = run(steps)
  assert lags.min() == 0 and lags.max() == 3
  # frames held: one from the post-reset write, one per substep, saturating at the ring
  assert (pushes == np.minimum(np.arange(steps)[:, None] + 2, 3)).all()
  # every column of a group holds the group's lag
  assert (eng.lag[:, 0:cols[1]] == eng.lag[:, 0:1]).all()
  counts = np.bincount(lags[:, :, 0].ravel(), minlength=4)
  chi2 = float(((counts - counts.mean()) ** 2 / counts.mean()).sum())
  print(f"lag histogram {counts.tolist()}, chi-square {chi2:.2f}")
  assert chi2 < 30.66
  assert (lags[:, 0, 0] != lags[:, 1, 0]).any()  # two worlds
  assert (lags[:, :, 0] != lags[:, :, 1]).any()  # two groups of one world
  # a new episode of every world does not repeat the last one's sequence (draws counts on)
  r.load(q, qv)
  assert int(eng.draws.min()) == steps
  again, _ = run(50)
  assert (again[:, :, 0] != lags[:50, :, 0]).mean() > 0.5
  assert np.isfinite(r.sim.data.qpos.cpu().numpy()).all()


# ------------------------------------------------------------------ setters, descriptor, envs
@guarded
def test_setters_act_on_the_engine(gpu_device):
  """set_gains / set_effort_limit on the actuator objects change the engine's torque with no
  further call (their tensors are views of the engine's buffers), equal to torch mode."""
  n = 64
  a = Rig(GO1, _pd, n, gpu_device, engine=True)
  b = Rig(GO1, _pd, n, gpu_device)
  q, qv = _states(a, seed=61)
  tgt, _ = _targets(a, q, seed=62)
  ids = torch.arange(0, n, 3, device=gpu_device)
  for r in (a, b):
    r.load(q, qv)
    r.target(tgt)
    act = r.robot.custom_actuators[0]
    act.set_gains(ids, kp=torch.full((len(ids),), 5.0, device=gpu_device))
    act.set_effort_limit(ids, torch.full((len(ids),), 3.0, device=gpu_device))
    r.env_step()
  _assert_equal(a.fields(), b.fields(), "after set_gains / set_effort_limit")
  c = a.sim.data.ctrl[ids][:, :8].abs()
  assert c.max() <= 3.0 and (c == 3.0).any()
  # the off switch: back to the torch path, same bits
  a.sim.clear_explicit_actuators()
  a.engine = None
  assert a.sim.explicit_actuators is None
  for r in (a, b):
    r.env_step()
  _assert_equal(a.fields(), b.fields(), "after clear_explicit_actuators")


@guarded
def test_bad_descriptors_are_refused(gpu_device):
  from mjlab_amd._lib import MjxError, lib
  from mjlab_amd.actuator import ActuatorDesc
  r = Rig(GO1, _delayed(0, 3), 8, gpu_device, engine=True)
  good = r.engine.desc
  L = lib()

  def refused(**edit):
    d = ActuatorDesc.from_buffer_copy(good)
    for k, v in edit.items():
      setattr(d, k, v)
    rc = L.mjx_sim_set_actuators(r.sim._sim, ctypes.addressof(d), None)
    return rc != 0, L.mjx_last_error().decode()

  nu = good.nu
  u8 = lambda v: ctypes.cast((ctypes.c_uint8 * nu)(*v), ctypes.c_void_p)
  keep = [u8([4] * nu), u8([5] * nu), u8([4] * nu), u8([0] * nu)]
  for edit in (dict(nworld=9), dict(nu=nu + 1), dict(ring_len=33), dict(ring_len=2), dict(kind=None),
               dict(kind=keep[0]), dict(max_lag=keep[1]), dict(min_lag=keep[2]), dict(kind=keep[3]),
               dict(kp=None), dict(position_target=None), dict(ring=None), dict(lag=None)):
    bad, why = refused(**edit)
    assert bad and "mjx_sim_set_actuators" in why, (edit, why)
  ok, _ = refused()
  assert not ok
  # an actuator the engine cannot run stays on the torch path with a reason
  rt = Rig(GO1, _delayed(0, 3, delay_hold_prob=0.5), 8, gpu_device)
  with pytest.raises(ValueError, match="hold"):
    rt.sim.set_explicit_actuators(rt.scene.entities.values())
  assert rt.sim.explicit_actuators is None
  rb = Rig(GO1, None, 8, gpu_device)
  with pytest.raises(ValueError, match="no explicit actuator"):
    rb.sim.set_explicit_actuators(rb.scene.entities.values())
  del MjxError


# ------------------------------------------------------------------ delayed builtin groups, hold
def _same(g):
  return g  # DelayedActuatorCfg around the asset's own builtin position group


@guarded
def test_delayed_builtin_group_engine_equals_torch(gpu_device):
  """Kind 1: the model's <position> actuators take their ctrl two substeps late."""
  a, _ = _twin_run(GO1, _delayed(2, 2, base=_same), 64, gpu_device)
  assert (a.engine.pushes == 2).all()


@guarded
def test_undelayed_builtin_pass_through_changes_nothing(gpu_device):
  """Lag 0 through the engine's pass-through equals the plain builtin scene, bit for bit."""
  n = 64
  a = Rig(GO1, _delayed(0, 0, base=_same), n, gpu_device, engine=True)
  b = Rig(GO1, None, n, gpu_device)
  q, qv = _states(a, seed=71)
  for r in (a, b):
    r.load(q, qv)
  for step in range(3):
    tgt, _ = _targets(a, q, seed=400 + step)
    for r in (a, b):
      r.target(tgt)
      r.env_step()
    _assert_equal(a.fields(), b.fields(), f"env step {step}")


@guarded
def test_held_lags_right_after_a_reset_equal_torch(gpu_device):
  """Random-range actuators ([0, 3]) with per-world lags pinned by set_lags(hold=True) right
  after a reset: a world with lag 3 holds one frame, then two, then three, so its read is
  clamped by the frames pushed in the first substeps -- equal to the torch ring bit for bit,
  the targets changing every substep.  The hold survives the pushes and ends at a reset."""
  n = 64
  make = _delayed(0, 3)
  a = Rig(GO1, make, n, gpu_device, engine=True, seed=9)
  b = Rig(GO1, make, n, gpu_device)
  q, qv = _states(a, seed=81)
  lags = torch.arange(n, device=gpu_device) % 4
  for r in (a, b):
    r.load(q, qv)
    for act in r.robot.custom_actuators:
      act.set_lags(lags, hold=True)
  for sub in range(6):
    tgt, _ = _targets(a, q, seed=500 + sub)
    for r in (a, b):
      r.target(tgt)
      r.env_step(nsub=1)
    assert (a.engine.pushes[:, 0] == min(sub + 2, 3)).all()
    _assert_equal(a.fields(), b.fields(), f"substep {sub}")
  assert (a.engine.lag == lags.view(-1, 1)).all()
  mask = torch.zeros(n, dtype=torch.bool, device=gpu_device)
  mask[::2] = True
  a.scene.reset_masked(mask)
  a.scene.write_data_to_sim(mask=mask)
  assert (a.engine.hold[mask] == 0).all() and (a.engine.hold[~mask] == 1).all()
  seen = []
  for _ in range(12):
    a.env_step(nsub=1)
    seen.append(a.engine.lag[:, 0].clone())
  seen = torch.stack(seen)
  assert (seen[:, ~mask] == lags[~mask]).all()  # still pinned
  assert (seen[:, mask].min(0).values != seen[:, mask].max(0).values).float().mean() > 0.9  # drawn again


# ------------------------------------------------------------------ 6. fused envs
ENV_N, ENV_STEPS, ENV_RESET_STEP = 64, 10, 3


def _env(task, make, device, fused, capture):
  """As tests/test_gpu_fused_history.py arranges its twins: same seed, corruption off, reset
  pose range zero, command and interval timers out of reach."""
  from mjlab_amd.envs import ManagerBasedRlEnv, load_env_cfg
  cfg = load_env_cfg(task, False)
  cfg.scene.num_envs = ENV_N
  cfg.seed = 3
  cfg.observations["policy"].enable_corruption = False
  cfg.events["reset_base"].params["pose_range"] = {}
  art = cfg.scene.entities["robot"].articulation
  art.actuators = tuple(make(i, g) for i, g in enumerate(art.actuators))
  e = ManagerBasedRlEnv(cfg, device=device)
  e.reset()
  e.enable_graph(capture=capture, fused=fused)
  e.command_manager.get_term("twist").time_left.fill_(1e6)
  for tl in e.event_manager._interval_time_left:
    tl.fill_(1e6)
  return e


def _command_columns(env, group):
  om = env.observation_manager
  off = 0
  for name, dim in zip(om._group_obs_term_names[group], om._group_obs_term_dim[group]):
    if name == "command":
      return slice(off, off + dim[0])
    off += dim[0]
  raise AssertionError("no command term")


@pytest.mark.parametrize("kind", ["ideal_pd", "delayed_pd"])
@pytest.mark.parametrize("task", [G1, GO1])
@guarded
def test_fused_env_runs_explicit_actuators_in_engine_mode(task, kind, gpu_device):
  """The velocity env with every actuator explicit builds the fused step and binds engine
  mode; ten captured env steps equal the unfused sync-free env in torch mode.  A third of the
  envs time out at step 3.  Physics state (qpos, qvel, ctrl, actuator_force) is compared bit
  for bit; observations and rewards at the fused tests' rtol = atol = 1e-4.  The velocity
  command is redrawn at a reset from different generators on the two paths (as
  test_gpu_fused_history notes), so its observation columns, and the rewards (which track
  it), are compared on the envs that have not been reset before the step."""
  make = (lambda i, g: _pd(g)) if kind == "ideal_pd" else (lambda i, g: _delayed(2, 2)(g))
  et = _env(task, make, gpu_device, fused=False, capture=False)
  ef = _env(task, make, gpu_device, fused=True, capture=True)
  assert ef._fused is not None, getattr(ef, "_fused_unsupported", "")
  eng = ef.sim.explicit_actuators
  assert eng is not None and ef._fused._engine_act is eng
  assert ef._fused._desc.ctrl and ctypes.addressof(ef._fused._desc.ctrl.contents) == eng.position_target.data_ptr()
  assert et._fused is None and et.sim.explicit_actuators is None
  n = ENV_N
  g = torch.Generator(device=gpu_device).manual_seed(0)
  nact = et.action_manager.total_action_dim
  was_reset = torch.zeros(n, dtype=torch.bool, device=gpu_device)
  for step in range(ENV_STEPS):
    if step == ENV_RESET_STEP:
      for e in (et, ef):
        e.episode_length_buf[::3] = e.max_episode_length - 1
    a = 0.3 * (2 * torch.rand(n, nact, device=gpu_device, generator=g) - 1)
    ot, rt, tt, ut, _ = et.step(a)
    of, rf, tf, uf, _ = ef.step(a)
    torch.cuda.synchronize()
    for k in ("qpos", "qvel", "ctrl", "actuator_force"):
      x, y = getattr(et.sim.data, k), getattr(ef.sim.data, k)
      d = (x.double() - y.double()).abs().max().item()
      print(f"{task} {kind} step {step}: {k} max |diff| {d:.3e}")
      assert torch.equal(x, y), (step, k, d)
    assert torch.equal(tt, tf) and torch.equal(ut, uf)
    fresh = ~was_reset
    torch.testing.assert_close(rt[fresh], rf[fresh], rtol=1e-4, atol=1e-4)
    was_reset |= tt | ut
    for grp in ("policy", "critic"):
      ok = torch.ones_like(ot[grp], dtype=torch.bool)
      ok[:, _command_columns(et, grp)] = ~was_reset[:, None]
      torch.testing.assert_close(torch.where(ok, ot[grp], 0).float(), torch.where(ok, of[grp], 0).float(),
                                 rtol=1e-4, atol=1e-4)
    if step == ENV_RESET_STEP:
      assert (tt | ut)[::3].all()
      if kind == "delayed_pd":  # the reset envs hold the one post-reset frame, the others a full ring
        assert (eng.pushes[::3] == 1).all() and (eng.pushes[1::3] == 2).all()
  assert ef._graph is not None and was_reset.any() and not was_reset.all()
  lim = ef.sim.data.ctrl.abs()
  assert (lim > 0).any()
  ef.enable_graph(capture=False, fused=False)  # dropping the fused step returns to torch mode
  assert ef._fused is None and ef.sim.explicit_actuators is None


@guarded
def test_fused_env_reports_a_mix_or_an_unsupported_policy(gpu_device):
  """A builtin / explicit mix on the action term's entity, or a delay policy the engine does
  not run, keeps the unfused sync-free step in torch mode and says why."""
  mix = _env(GO1, lambda i, g: _pd(g) if i == 0 else g, gpu_device, fused=True, capture=False)
  assert mix._fused is None and "mix of builtin and explicit" in mix._fused_unsupported
  assert mix.sim.explicit_actuators is None
  hold = _env(GO1, lambda i, g: _delayed(0, 3, delay_hold_prob=0.5)(g), gpu_device, fused=True, capture=False)
  assert hold._fused is None and "delay_hold_prob" in hold._fused_unsupported
  assert hold.sim.explicit_actuators is None
  nact = mix.action_manager.total_action_dim
  for e in (mix, hold):
    for _ in range(2):
      e.step(torch.zeros(ENV_N, nact, device=gpu_device))
    assert torch.isfinite(e.sim.data.qpos).all()
