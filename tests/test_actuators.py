"""Explicit actuators (mjlab_amd.actuator) on the CPU: the laws from hand-built commands, the
delay wrapper, the compiled <motor> group and the entity wiring.  No simulation is created;
the engine form of the laws is checked on the GPU (tests/test_gpu_actuators.py).

The known answers are those of the reference's tests/test_pd_actuator.py,
test_dc_actuator.py and test_delayed_actuator.py."""

import ctypes
import os
import warnings
from types import SimpleNamespace

import pytest
import torch

from mjlab_amd.actuator import (ActuatorCmd, DcMotorActuatorCfg, DelayedActuator, DelayedActuatorCfg,
                                IdealPdActuator, IdealPdActuatorCfg, engine_unsupported)

N = 4


def _data(n=N):
  return SimpleNamespace(qpos=torch.zeros(n, 1))


def _build(cfg, n=N, joints=("joint1", "joint2")):
  act = cfg.build(None, list(range(len(joints))), list(joints))
  act._ctrl_ids_list = list(range(len(joints)))
  act.initialize(None, None, _data(n), "cpu")
  return act


def _cmd(pt=0.0, vt=0.0, ft=0.0, q=0.0, qd=0.0, n=N, nj=2):
  f = lambda v: torch.as_tensor(v, dtype=torch.float32).expand(n, nj).clone()
  return ActuatorCmd(position_target=f(pt), velocity_target=f(vt), effort_target=f(ft),
                     joint_pos=f(q), joint_vel=f(qd))


def _pd(**kw):
  kw.setdefault("joint_names_expr", ("joint.*",))
  kw.setdefault("stiffness", 50.0)
  kw.setdefault("damping", 5.0)
  return IdealPdActuatorCfg(**kw)


def _dc(effort_limit, kp=100.0, kd=0.0, sat=20.0, vlim=30.0):
  with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    return DcMotorActuatorCfg(joint_names_expr=("joint.*",), stiffness=kp, damping=kd,
                              effort_limit=effort_limit, saturation_effort=sat, velocity_limit=vlim)


# ------------------------------------------------------------------ ideal PD
def test_pd_known_answers():
  act = _build(_pd())
  # kp (pt - q) + kd (vt - qd) = 50 * (1 - 0.2) + 5 * (0 - 0.5) = 37.5
  out = act.compute(_cmd(pt=1.0, q=0.2, qd=0.5))
  assert torch.allclose(out, torch.full((N, 2), 37.5))
  assert out.shape == (N, 2) and act.ctrl_ids.tolist() == [0, 1] and act.joint_ids.tolist() == [0, 1]


def test_pd_feed_forward_adds_to_the_pd_term():
  act = _build(_pd())
  out = act.compute(_cmd(pt=1.0, vt=2.0, ft=3.0, q=0.0, qd=0.0))
  assert torch.allclose(out, torch.full((N, 2), 50.0 + 10.0 + 3.0))


def test_pd_clamps_to_the_effort_limit_both_signs():
  act = _build(_pd(effort_limit=10.0))
  assert torch.equal(act.compute(_cmd(pt=1.0)), torch.full((N, 2), 10.0))
  assert torch.equal(act.compute(_cmd(pt=-1.0)), torch.full((N, 2), -10.0))
  assert torch.allclose(act.compute(_cmd(pt=0.1)), torch.full((N, 2), 5.0))


def test_set_gains_and_effort_limit_per_env():
  act = _build(_pd(effort_limit=100.0))
  act.set_gains(torch.tensor([1, 3]), kp=torch.tensor([10.0, 20.0]), kd=torch.tensor([[1.0, 2.0], [3.0, 4.0]]))
  assert act.stiffness[:, 0].tolist() == [50.0, 10.0, 50.0, 20.0]
  assert act.damping[3].tolist() == [3.0, 4.0] and act.damping[0].tolist() == [5.0, 5.0]
  assert torch.equal(act.default_stiffness, torch.full((N, 2), 50.0))
  out = act.compute(_cmd(pt=1.0))
  assert out[:, 0].tolist() == [50.0, 10.0, 50.0, 20.0]
  act.set_effort_limit(slice(0, 1), torch.tensor([7.0]))
  assert act.compute(_cmd(pt=1.0))[0].tolist() == [7.0, 7.0]


# ------------------------------------------------------------------ DC motor
def test_dc_stall_torque():
  act = _build(_dc(20.0))
  assert torch.allclose(act.compute(_cmd(pt=1.0, qd=0.0)), torch.full((N, 2), 20.0))


def test_dc_zero_torque_at_the_velocity_limit():
  act = _build(_dc(20.0))
  assert torch.allclose(act.compute(_cmd(pt=1.0, qd=30.0)), torch.zeros(N, 2), atol=1e-5)


@pytest.mark.parametrize("qd,pt,expected", [(15.0, 1.0, 10.0), (-15.0, -1.0, -10.0)])
def test_dc_half_torque_at_half_speed(qd, pt, expected):
  act = _build(_dc(20.0))
  assert torch.allclose(act.compute(_cmd(pt=pt, qd=qd)), torch.full((N, 2), expected), rtol=1e-4)


def test_dc_negative_velocity_raises_the_forward_limit_to_the_rating():
  # moving backwards the torque-speed line allows more than the stall torque; effort_limit caps it
  act = _build(_dc(20.0))
  assert torch.allclose(act.compute(_cmd(pt=1.0, qd=-15.0)), torch.full((N, 2), 20.0))


def test_dc_effort_limit_constrains_the_output():
  act = _build(_dc(5.0))
  assert torch.allclose(act.compute(_cmd(pt=1.0, qd=0.0)), torch.full((N, 2), 5.0))


def test_dc_corner_velocity():
  act = _build(_dc(10.0))
  corner = 30.0 * (1.0 - 10.0 / 20.0)  # the torque-speed line meets effort_limit here
  assert torch.allclose(act.compute(_cmd(pt=2.0, qd=corner)), torch.full((N, 2), 10.0), rtol=1e-4)
  assert torch.allclose(act._vel_at_effort_lim, torch.full((N, 2), 30.0 * (1.0 + 10.0 / 20.0)))


def test_dc_warns_for_an_infinite_effort_limit():
  with pytest.warns(UserWarning, match="effort_limit is set to inf"):
    DcMotorActuatorCfg(joint_names_expr=("j",), stiffness=100.0, damping=10.0, saturation_effort=20.0,
                       velocity_limit=30.0)


def test_dc_warns_when_the_effort_limit_exceeds_saturation():
  with pytest.warns(UserWarning, match="exceeds saturation_effort"):
    DcMotorActuatorCfg(joint_names_expr=("j",), stiffness=100.0, damping=10.0, saturation_effort=20.0,
                       velocity_limit=30.0, effort_limit=25.0)


# ------------------------------------------------------------------ delay
def _delayed(lo, hi, target="position", kp=1.0, **kw):
  return _build(DelayedActuatorCfg(base_cfg=_pd(stiffness=kp, damping=0.0), delay_target=target,
                                   delay_min_lag=lo, delay_max_lag=hi, **kw))


def test_delayed_cfg_takes_the_base_cfgs_joints():
  cfg = DelayedActuatorCfg(base_cfg=_pd(armature=0.01), delay_max_lag=2)
  assert cfg.joint_names_expr == ("joint.*",) and cfg.armature == 0.01
  act = _build(cfg)
  assert isinstance(act, DelayedActuator) and isinstance(act.base_actuator, IdealPdActuator)
  assert act.ctrl_ids.tolist() == [0, 1]


def test_constant_delay():
  act = _delayed(2, 2)
  outs = [float(act.compute(_cmd(pt=float(t)))[0, 0]) for t in range(1, 7)]
  # lag 2, clamped to the frames held: targets 1, 1, 1, 2, 3, 4
  assert outs == [1.0, 1.0, 1.0, 2.0, 3.0, 4.0]


def test_delay_reset_clears_the_rows_history():
  act = _delayed(2, 2)
  for t in range(1, 5):
    act.compute(_cmd(pt=float(t)))
  act.reset(torch.tensor([1]))
  out = act.compute(_cmd(pt=9.0))
  assert float(out[1, 0]) == 9.0  # a fresh row reads what it was just given
  assert float(out[0, 0]) == 3.0  # the others go on: frame 5 - 2
  act.reset()
  assert float(act.compute(_cmd(pt=7.0))[0, 0]) == 7.0


def test_delay_of_several_targets():
  act = _build(DelayedActuatorCfg(base_cfg=_pd(stiffness=1.0, damping=1.0),
                                  delay_target=("position", "velocity", "effort"),
                                  delay_min_lag=1, delay_max_lag=1))
  act.compute(_cmd(pt=1.0, vt=10.0, ft=100.0))
  out = act.compute(_cmd(pt=2.0, vt=20.0, ft=200.0))
  assert float(out[0, 0]) == 111.0  # all three one step late
  only_pos = _delayed(1, 1)
  only_pos.compute(_cmd(pt=1.0, ft=100.0))
  assert float(only_pos.compute(_cmd(pt=2.0, ft=200.0))[0, 0]) == 201.0


def test_delay_target_is_validated():
  with pytest.raises(ValueError):
    DelayedActuatorCfg(base_cfg=_pd(), delay_target="torque")


def test_set_lags_all_subset_and_clamped():
  # a long update period holds the lags that set_lags wrote
  act = _delayed(0, 3, delay_update_period=1000, delay_per_env_phase=False)
  for t in range(1, 6):
    act.compute(_cmd(pt=float(t)))
  buf = act._delay_buffers["position"]
  act.set_lags(torch.tensor(2))
  assert buf.current_lags.tolist() == [2, 2, 2, 2]
  act.set_lags(torch.tensor([0, 3]), torch.tensor([1, 2]))
  assert buf.current_lags.tolist() == [2, 0, 3, 2]
  act.set_lags(torch.tensor([9, -4]), torch.tensor([0, 3]))
  assert buf.current_lags.tolist() == [3, 0, 3, 0]  # clamped to [min_lag, max_lag]
  out = act.compute(_cmd(pt=6.0))
  assert out[:, 0].tolist() == [3.0, 6.0, 3.0, 6.0]


def test_set_lags_is_overwritten_without_a_hold():
  act = _delayed(1, 1)
  act.compute(_cmd(pt=1.0))
  act.set_lags(torch.tensor(0))  # clamped to 1 already; and every compute redraws in [1, 1]
  assert float(act.compute(_cmd(pt=2.0))[0, 0]) == 1.0
  assert act._delay_buffers["position"].current_lags.tolist() == [1] * N


def test_compute_with_a_mask_leaves_the_other_rows_untouched():
  act = _delayed(2, 2)
  for t in range(1, 5):
    act.compute(_cmd(pt=float(t)))
  buf = act._delay_buffers["position"]
  before = [t.clone() for t in (buf._buffer.buffer, buf._buffer.num_pushes, buf.current_lags, buf._step_count)]
  mask = torch.tensor([True, False, True, False])
  out = act.compute(_cmd(pt=5.0), mask=mask)
  after = (buf._buffer.buffer, buf._buffer.num_pushes, buf.current_lags, buf._step_count)
  for b, a in zip(before, after):
    assert torch.equal(a[~mask], b[~mask])
  assert buf._buffer.num_pushes.tolist() == [5, 4, 5, 4]
  assert out[:, 0].tolist() == [3.0, 2.0, 3.0, 2.0]  # stepped rows: frame 5 - 2; held rows: 4 - 2
  # the next unmasked step is what the held rows would have seen without the masked call
  assert act.compute(_cmd(pt=6.0))[:, 0].tolist() == [4.0, 3.0, 4.0, 3.0]


def test_masked_first_compute_leaves_the_other_rows_empty():
  act = _delayed(1, 1)
  mask = torch.tensor([True, False, False, False])
  act.compute(_cmd(pt=5.0), mask=mask)
  assert act._delay_buffers["position"]._buffer.num_pushes.tolist() == [1, 0, 0, 0]
  assert act.compute(_cmd(pt=6.0))[:, 0].tolist() == [5.0, 6.0, 6.0, 6.0]


def test_engine_mode_supports_position_delay_without_hold_or_period():
  assert engine_unsupported(_build(_pd())) is None
  assert engine_unsupported(_build(_dc(10.0))) is None
  assert engine_unsupported(_delayed(0, 3)) is None
  assert "delay_target" in engine_unsupported(_delayed(0, 3, target=("position", "effort")))
  assert "hold" in engine_unsupported(_delayed(0, 3, delay_hold_prob=0.5))
  assert "period" in engine_unsupported(_delayed(0, 3, delay_update_period=4))


# ------------------------------------------------------------------ compiler / entity
def _go1_cfg(make):
  from mjlab_amd.envs import load_env_cfg
  cfg = load_env_cfg("Mjlab-Velocity-Flat-Unitree-Go1")
  cfg.scene.num_envs = N
  art = cfg.scene.entities["robot"].articulation
  art.actuators = tuple(make(g) for g in art.actuators)
  return cfg


def _as_pd(g, **kw):
  return IdealPdActuatorCfg(joint_names_expr=g.joint_names_expr, stiffness=g.stiffness,
                            damping=g.damping, effort_limit=g.effort_limit, armature=g.armature, **kw)


def test_ideal_pd_cfg_compiles_to_motors():
  import numpy as np
  from mjlab_amd.scene import Scene
  builtin = Scene(_go1_cfg(lambda g: g).scene, "cpu").compile()
  m = Scene(_go1_cfg(_as_pd).scene, "cpu").compile()
  assert m.nu == builtin.nu == 12 and m.names["actuator"] == builtin.names["actuator"]
  lim = np.asarray(builtin.actuator_forcerange)[:, 1]
  assert (lim > 0).all()
  for rng in (np.asarray(m.actuator_forcerange), np.asarray(m.actuator_ctrlrange)):
    assert np.array_equal(rng, np.stack([-lim, lim], axis=1))
  assert np.asarray(m.actuator_ctrllimited).all() and np.asarray(m.actuator_forcelimited).all()
  # a <motor>: force = ctrl (fixed unit gain, no bias), and the joints keep the armature
  assert np.array_equal(np.asarray(m.actuator_gainprm)[:, 0], np.ones(12))
  assert not np.asarray(m.actuator_biasprm).any()
  assert np.array_equal(np.asarray(m.dof_armature), np.asarray(builtin.dof_armature))
  # the delay wrapper compiles to what its base compiles to
  md = Scene(_go1_cfg(lambda g: DelayedActuatorCfg(base_cfg=_as_pd(g), delay_max_lag=2)).scene,
             "cpu").compile()
  assert np.array_equal(np.asarray(md.actuator_ctrlrange), np.asarray(m.actuator_ctrlrange))


def test_frictionloss_stays_refused():
  from mjlab_amd.scene import Scene
  with pytest.raises(NotImplementedError, match="frictionloss"):
    Scene(_go1_cfg(lambda g: _as_pd(g, frictionloss=0.1)).scene, "cpu").compile()


def test_other_actuator_cfg_types_stay_a_type_error():
  from mjlab_amd.scene import Scene
  with pytest.raises(TypeError, match="unsupported actuator cfg"):
    Scene(_go1_cfg(lambda g: object()).scene, "cpu").compile()


def test_entity_writes_the_explicit_torque_to_ctrl():
  from mjlab_amd.scene import Scene
  scene = Scene(_go1_cfg(_as_pd).scene, "cpu")
  m = scene.compile()
  torch.manual_seed(0)
  data = SimpleNamespace(qpos=torch.randn(N, m.nq) * 0.1, qvel=torch.randn(N, m.nv),
                         ctrl=torch.zeros(N, m.nu), time=torch.zeros(N),
                         sensordata=torch.zeros(N, m.nsensordata))
  scene.initialize(m, None, data)
  robot = scene["robot"]
  acts = robot.custom_actuators
  assert [len(a.joint_names) for a in acts] == [8, 4]
  assert sorted(c for a in acts for c in a.ctrl_ids.tolist()) == list(range(12))
  target = torch.randn(N, 12) * 1.5  # errors on both sides of effort_limit / kp (~1 rad)
  bound = free = 0
  robot.set_joint_position_target(target)
  scene.write_data_to_sim()
  for a in acts:
    j = a.joint_ids
    kp, kd, lim = a.cfg.stiffness, a.cfg.damping, a.cfg.effort_limit
    want = (kp * (target[:, j] - robot.data.joint_pos[:, j]) - kd * robot.data.joint_vel[:, j]).clamp(-lim, lim)
    got = data.ctrl[:, robot.indexing.ctrl_ids[a.ctrl_ids]]
    assert torch.allclose(got, want, atol=1e-4)
    assert [robot.actuator_names[c] for c in a.ctrl_ids.tolist()] == a.joint_names
    bound += int((got.abs() == lim).sum())
    free += int((got.abs() < lim).sum())
  assert bound > 0 and free > 0  # the clamp binds in places


def test_entity_reset_resets_the_delay_buffers():
  from mjlab_amd.scene import Scene
  scene = Scene(_go1_cfg(lambda g: DelayedActuatorCfg(base_cfg=_as_pd(g), delay_min_lag=1,
                                                      delay_max_lag=1)).scene, "cpu")
  m = scene.compile()
  data = SimpleNamespace(qpos=torch.zeros(N, m.nq), qvel=torch.zeros(N, m.nv), ctrl=torch.zeros(N, m.nu),
                         time=torch.zeros(N), sensordata=torch.zeros(N, m.nsensordata))
  scene.initialize(m, None, data)
  robot = scene["robot"]
  for _ in range(3):
    scene.write_data_to_sim()
  bufs = [a._delay_buffers["position"]._buffer for a in robot.custom_actuators]
  assert all(b.num_pushes.tolist() == [3] * N for b in bufs)
  robot.reset(torch.tensor([0]))
  assert all(b.num_pushes.tolist() == [0, 3, 3, 3] for b in bufs)
  mask = torch.tensor([False, True, False, False])
  scene.reset_masked(mask)
  assert all(b.num_pushes.tolist() == [0, 0, 3, 3] for b in bufs)
  scene.write_data_to_sim(mask=mask)  # the sync-free env's post-reset write: only the reset rows
  assert all(b.num_pushes.tolist() == [0, 1, 3, 3] for b in bufs)


# ------------------------------------------------------------------ C ABI
def test_bad_descriptors_return_an_error_code():
  """mjx_sim_set_actuators checks the descriptor's own consistency before it looks at the sim,
  so every refusal below is reached without a GPU; a consistent descriptor then fails on the
  null sim."""
  lib_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mjlab-1_amd",
                          "mjlab_amd", "libmjx355.so")
  if not os.path.exists(lib_path):
    pytest.skip("libmjx355.so not built (run __graft_entry__.build())")
  from mjlab_amd.actuator import ActuatorDesc
  L = ctypes.CDLL(lib_path)
  L.mjx_last_error.restype = ctypes.c_char_p
  L.mjx_actuator_desc_size.restype = ctypes.c_size_t
  assert L.mjx_actuator_desc_size() == ctypes.sizeof(ActuatorDesc)
  L.mjx_sim_set_actuators.argtypes = [ctypes.c_void_p] * 3
  nu, n, ring = 3, 2, 4
  u8 = lambda v: ctypes.cast((ctypes.c_uint8 * nu)(*v), ctypes.c_void_p)
  tables = dict(kind=u8([1, 2, 3]), min_lag=u8([0, 1, 0]), max_lag=u8([3, 1, 0]), group=u8([0, 1, 2]))
  store = (ctypes.c_float * (n * ring * nu))()  # never read: every call fails before a launch
  somewhere = ctypes.cast(store, ctypes.c_void_p)

  def call(**edit):
    d = ActuatorDesc()
    d.nworld, d.nu, d.ring_len, d.seed = n, nu, ring, 1
    for k, v in tables.items():
      setattr(d, k, v)
    for k in ("kp", "kd", "effort_limit", "saturation_effort", "velocity_limit", "corner_velocity",
              "position_target", "velocity_target", "effort_target", "ring", "lag", "pushes", "draws"):
      setattr(d, k, somewhere)
    for k, v in edit.items():
      setattr(d, k, v)
    rc = L.mjx_sim_set_actuators(None, ctypes.byref(d), None)
    return rc, L.mjx_last_error().decode()

  for edit, why in ((dict(nworld=0), "nworld"), (dict(nu=0), "nu"), (dict(nu=65), "nu"),
                    (dict(ring_len=-1), "ring_len"), (dict(ring_len=33), "ring_len"),
                    (dict(kind=None), "null kind"), (dict(group=None), "null kind"),
                    (dict(kind=u8([4, 2, 3])), "kind must be"),
                    (dict(min_lag=u8([0, 2, 0])), "min_lag > max_lag"),
                    (dict(ring_len=2), "exceeds ring_len"),
                    (dict(kind=u8([0, 2, 3])), "builtin actuator cannot be delayed"),
                    (dict(kind=u8([0, 0, 0]), max_lag=u8([0, 0, 0]), min_lag=u8([0, 0, 0])),
                     "no explicit actuator"),
                    (dict(position_target=None), "position_target"), (dict(kp=None), "gain"),
                    (dict(effort_target=None), "gain"), (dict(velocity_limit=None), "DC motor"),
                    (dict(ring=None), "delay buffer"), (dict(draws=None), "delay buffer")):
    rc, msg = call(**edit)
    assert rc != 0 and "mjx_sim_set_actuators" in msg and why in msg, (edit, msg)
  rc, msg = call()  # consistent (hold may be null): only the sim is missing
  assert rc != 0 and "null sim" in msg
  rc, msg = call(kind=u8([1, 1, 1]), kp=None, kd=None, effort_limit=None)  # delayed builtins need no gains
  assert rc != 0 and "null sim" in msg
  assert L.mjx_sim_set_actuators(None, None, None) != 0 and b"null sim" in L.mjx_last_error()


# ------------------------------------------------------------------ hold, delayed builtin groups
def test_set_lags_with_hold_pins_the_lag_until_the_reset():
  act = _delayed(0, 3)
  for t in range(1, 6):
    act.compute(_cmd(pt=float(t)))
  act.set_lags(torch.tensor([3, 1]), torch.tensor([0, 2]), hold=True)
  buf = act._delay_buffers["position"]
  for t in range(6, 30):
    out = act.compute(_cmd(pt=float(t)))
    assert float(out[0, 0]) == t - 3 and float(out[2, 0]) == t - 1
  assert buf.current_lags[0] == 3 and buf.current_lags[2] == 1
  seen = set()
  for t in range(30, 70):  # rows 1 and 3 redraw on [0, 3] all along
    act.compute(_cmd(pt=float(t)))
    seen.add(int(buf.current_lags[1]))
  assert len(seen) > 1
  act.reset(torch.tensor([0]))  # a reset releases the hold
  lags = set()
  for t in range(70, 110):
    act.compute(_cmd(pt=float(t)))
    lags.add(int(buf.current_lags[0]))
  assert len(lags) > 1 and buf.current_lags[2] == 1


def test_delayed_builtin_position_group_passes_the_late_target_through():
  from mjlab_amd.actuator import KIND_DELAYED, BuiltinActuator, engine_kind
  from mjlab_amd.compiler.model import PositionActuatorGroup, VelocityActuatorGroup
  grp = PositionActuatorGroup(("joint.*",), stiffness=20.0, damping=1.0, effort_limit=5.0, armature=0.02)
  cfg = DelayedActuatorCfg(base_cfg=grp, delay_min_lag=2, delay_max_lag=2)
  assert cfg.joint_names_expr == ("joint.*",) and cfg.armature == 0.02
  assert cfg.compile_group() is grp  # the model keeps its <position> actuators
  act = _build(cfg)
  assert isinstance(act.base_actuator, BuiltinActuator) and engine_kind(act.base_actuator) == KIND_DELAYED
  assert engine_unsupported(act) is None
  outs = [float(act.compute(_cmd(pt=float(t), q=0.3, qd=0.7))[0, 0]) for t in range(1, 6)]
  assert outs == [1.0, 1.0, 1.0, 2.0, 3.0]  # ctrl is the target itself, two steps late
  vel = _build(DelayedActuatorCfg(base_cfg=VelocityActuatorGroup(("joint.*",), damping=1.0),
                                  delay_target="velocity", delay_max_lag=1))
  assert float(vel.compute(_cmd(pt=1.0, vt=4.0))[0, 0]) == 4.0
  assert "no engine form" in engine_unsupported(vel)
  with pytest.raises(TypeError, match="base_cfg"):
    _build(DelayedActuatorCfg(base_cfg=SimpleNamespace(joint_names_expr=("j",), armature=0.0,
                                                       frictionloss=0.0)))


def test_delay_buffer_masked_append_and_compute():
  from mjlab_amd.buffers import DelayBuffer
  buf = DelayBuffer(min_lag=1, max_lag=1, batch_size=3)
  for t in (1.0, 2.0):
    buf.append(torch.full((3, 1), t))
    buf.compute()
  mask = torch.tensor([True, False, True])
  buf.append(torch.full((3, 1), 3.0), mask)
  out = buf.compute(mask)
  assert out[:, 0].tolist() == [2.0, 1.0, 2.0]
  assert buf._buffer.num_pushes.tolist() == [3, 2, 3] and buf._step_count.tolist() == [3, 2, 3]
