"""Learned (MLP) actuators on the GPU: the engine's phase-A network evaluation
(mjx_sim_set_actuator_nets, csrc/engine_impl.h net_torque / net_push) and the torch path
(mjlab_amd.actuator.LearnedMlpActuator) against the fp64 reference of tests/learned_ref.py,
whose docstring derives the bound |ctrl - ctrl_ref| <= e_t + u |ctrl_ref| asserted here.

Scenes are the Go1 (64 worlds) and G1 (96 worlds) flat velocity scenes with the builtin
position groups replaced by LearnedMlpActuatorCfg; the networks are seeded random MLPs written
to a temporary directory.  Network shapes: (a) H = 1, a single Linear(2, 1); (b) H = 3,
6-32-32-32-1 softsign (maximum depth and width); (c) H = 8, 16-5-1 tanh, vel_pos (maximum
history, odd width); (d) H = 3, 6-8-1 elu; (e) G1 with (b) and (c) on different groups and one
group an ideal PD (one wave holds mixed kinds and networks); (f) (b) behind a fixed delay of 2.
torque_scale is about 3 effort_limit (G1's two largest limits share 330, so that its six groups
need four networks) on networks whose output is mostly within +-0.3, so the DC clip binds for
part of the actuators and the robots are not thrown about.  The stall torque is 2 effort_limit:
the torque-speed line then meets the rating at an exactly representable corner (1.5
velocity_limit), so no limit exceeds effort_limit by a rounding and actuator_force == ctrl can
be asserted bit for bit.  The no-load speed is 2 rad/s: at the seeded joint speeds (a few rad/s)
the torque-speed line binds for part of the actuators, and it brakes the joints the random
networks push.

The history the engine keeps is compared bit for bit with a host mirror built from the
engine's own read-back states.  The fault rule is that of tests/test_gpu_actuators.py (shared
flag: after a GPU fault every later test fails without touching the GPU)."""

from __future__ import annotations

import ctypes
import warnings

import numpy as np
import pytest
import torch
from torch import nn

import learned_ref as lr
from test_gpu_actuators import (ENV_N, ENV_RESET_STEP, ENV_STEPS, FIELDS, G1, GO1, Rig, _assert_equal,
                                _command_columns, _env, _joint_q, _joint_v, _states, guarded)

pytestmark = pytest.mark.gpu

F32 = np.float32
SHAPES = {  # name: (history, widths, activation, input order)
    "a": (1, [2, 1], nn.ReLU, "pos_vel"),
    "b": (3, [6, 32, 32, 32, 1], nn.Softsign, "pos_vel"),
    "c": (8, [16, 5, 1], nn.Tanh, "vel_pos"),
    "d": (3, [6, 8, 1], nn.ELU, "pos_vel"),
}
OUT_GAIN = {"a": 0.35, "b": 0.9, "c": 0.35, "d": 0.35}  # last-layer scale: |output| mostly below 0.5
POS_SCALE, VEL_SCALE, DC_SAT, DC_VLIM = 2.5, 0.15, 2.0, 2.0


def _tscale(limit):
  return 330.0 if limit >= 80.0 else 3.0 * limit


@pytest.fixture(scope="module")
def nets(tmp_path_factory):
  """name -> (file, layers of the fp64 reference), written once."""
  d = tmp_path_factory.mktemp("nets")
  out = {}
  for k, (name, (H, widths, act, _)) in enumerate(SHAPES.items()):
    seq = lr.make_net(widths, act, seed=40 + k, out_gain=OUT_GAIN[name])
    out[name] = (lr.save_net(seq, d / f"{name}.pt"), lr.layers_of(seq))
  # shape (b) with a small output for the env test: the robots stay up for its ten steps
  seq = lr.make_net(SHAPES["b"][1], SHAPES["b"][2], seed=50, out_gain=0.1)
  out["b_small"] = (lr.save_net(seq, d / "b_small.pt"), lr.layers_of(seq))
  bad = nn.Sequential(nn.Linear(6, 8), nn.LayerNorm(8), nn.Linear(8, 1))
  out["layernorm"] = (lr.save_net(bad, d / "layernorm.pt"), None)
  return out


def _learned(nets, name, lag=0, tscale=_tscale):
  def make(g):
    from mjlab_amd.actuator import DelayedActuatorCfg, LearnedMlpActuatorCfg
    H, _, _, order = SHAPES.get(name, SHAPES["b"])
    with warnings.catch_warnings():
      warnings.simplefilter("ignore")
      cfg = LearnedMlpActuatorCfg(
          joint_names_expr=g.joint_names_expr, network_file=nets[name][0], pos_scale=POS_SCALE,
          vel_scale=VEL_SCALE, torque_scale=tscale(g.effort_limit), input_order=order, history_length=H,
          effort_limit=g.effort_limit, saturation_effort=DC_SAT * g.effort_limit,
          velocity_limit=DC_VLIM, armature=g.armature)
    cfg.shape = name
    return DelayedActuatorCfg(base_cfg=cfg, delay_min_lag=lag, delay_max_lag=lag) if lag else cfg
  return make


def _mixed(nets):
  """(e): groups in turn on network (b), network (c) and an ideal PD."""
  count = [0]

  def make(g):
    from mjlab_amd.actuator import IdealPdActuatorCfg
    i, count[0] = count[0], count[0] + 1
    if i % 3 == 2:
      return IdealPdActuatorCfg(joint_names_expr=g.joint_names_expr, stiffness=g.stiffness,
                                damping=g.damping, effort_limit=g.effort_limit, armature=g.armature)
    return _learned(nets, "bc"[i % 3])(g)
  return make


CASES = {"a": (GO1, 64, "a", 0), "b": (GO1, 64, "b", 0), "c": (GO1, 64, "c", 0), "d": (G1, 96, "d", 0),
         "e": (G1, 96, None, 0), "f": (GO1, 64, "b", 2)}


def _rig(nets, case, device, engine=True, capacity=None):
  task, n, shape, lag = CASES[case]
  make = _mixed(nets) if shape is None else _learned(nets, shape, lag)
  return Rig(task, make, n, device, capacity=capacity, engine=engine)


def _groups(rig):
  """[(entity-local actuator ids, cfg, lag)] of the learned actuators."""
  from mjlab_amd.actuator import DelayedActuator, LearnedMlpActuator
  out = []
  for act in rig.robot.custom_actuators:
    base = act.base_actuator if isinstance(act, DelayedActuator) else act
    if isinstance(base, LearnedMlpActuator):
      lag = act.cfg.delay_max_lag if isinstance(act, DelayedActuator) else 0
      out.append((np.asarray(act._ctrl_ids_list), base.cfg, lag))
  return out


def _gid(rig):
  return rig.robot.indexing.ctrl_ids.cpu().numpy()


def _rand_targets(rig, seed):
  """Joint-order targets within +-0.6 rad of the joint positions, and their actuator-order view."""
  rng = np.random.default_rng(seed)
  qa = _joint_q(rig, rig.sim.data.qpos.cpu().numpy())
  tgt_act = (qa + rng.uniform(-0.6, 0.6, qa.shape)).astype(F32)
  tgt = np.zeros((rig.n, rig.robot.num_joints), F32)
  tgt[:, rig.robot._act_joint_local] = tgt_act
  return tgt, tgt_act


class Mirror:
  """Host mirror of the engine's history, in entity actuator order: `hist` [n, Hm, 2, na]
  oldest first, `pushes` [n, na], and per delayed group the position targets pushed so far."""

  def __init__(self, rig):
    self.rig, self.groups, self.gid = rig, _groups(rig), _gid(rig)
    self.Hm = max(c.history_length for _, c, _ in self.groups) - 1
    na = len(self.gid)
    self.hist = np.zeros((rig.n, self.Hm, 2, na), F32)
    self.pushes = np.zeros((rig.n, na), np.int32)
    # per group: the last position targets pushed to the delay ring, [n, 4, cols] oldest first
    self.tring = [np.zeros((rig.n, 4, len(c)), F32) for c, _, _ in self.groups]
    self.tpush = np.zeros(rig.n, np.int64)

  def copy(self):
    m = Mirror.__new__(Mirror)
    m.__dict__.update(self.__dict__)
    m.hist, m.pushes, m.tpush = self.hist.copy(), self.pushes.copy(), self.tpush.copy()
    m.tring = [t.copy() for t in self.tring]
    return m

  def state(self):
    d = self.rig.sim.data
    return (_joint_q(self.rig, d.qpos.cpu().numpy()).astype(F32),
            _joint_v(self.rig, d.qvel.cpu().numpy()).astype(F32))

  def late(self, k, tgt_act):
    """The (possibly delayed) target of group k at this substep."""
    cols, _, lag = self.groups[k]
    pt = tgt_act[:, cols].copy()
    held = np.minimum(lag, self.tpush)
    for w in np.nonzero(held > 0)[0]:
      pt[w] = self.tring[k][w, -held[w]]
    return pt

  def frames(self, k, tgt_act, q, qd):
    """Lag-indexed frames of group k: the current one, then the held history (lag clamped)."""
    cols, cfg, _ = self.groups[k]
    H = cfg.history_length
    pe = np.zeros((self.rig.n, len(cols), H), F32)
    v = np.zeros_like(pe)
    pe[..., 0] = self.late(k, tgt_act) - q[:, cols]
    v[..., 0] = qd[:, cols]
    for j in range(1, H):
      kk = np.minimum(j, self.pushes[:, cols])
      src = self.hist[np.arange(self.rig.n)[:, None], np.clip(self.Hm - kk, 0, self.Hm - 1), :, cols]
      pe[..., j] = np.where(kk > 0, src[..., 0], pe[..., 0])
      v[..., j] = np.where(kk > 0, src[..., 1], v[..., 0])
    return pe, v

  def push(self, tgt_act, q, qd):
    """One integrated substep at state (q, qd) with targets tgt_act."""
    rows = np.ones(self.rig.n, bool)
    for k, (cols, cfg, lag) in enumerate(self.groups):
      h = cfg.history_length - 1
      pe = self.late(k, tgt_act) - q[:, cols]
      if h > 0:
        lo = self.Hm - h
        new = self.hist.copy()
        new[:, lo:self.Hm - 1, :, cols] = self.hist[:, lo + 1:, :, cols]
        new[:, -1, 0, cols] = pe
        new[:, -1, 1, cols] = qd[:, cols]
        self.hist[rows] = new[rows]
        self.pushes[np.ix_(rows, cols)] = np.minimum(self.pushes[np.ix_(rows, cols)] + 1, h)
    for k, (cols, _, lag) in enumerate(self.groups):
      self.tring[k] = np.concatenate([self.tring[k][:, 1:], tgt_act[:, None, cols]], axis=1)
    self.tpush += 1

  def prime(self, rows, tgt_act, q, qd):
    """A reset of `rows` and the post-reset frame."""
    self.hist[rows] = 0
    self.pushes[rows] = 0
    self.tpush[rows] = 0
    for k, (cols, cfg, lag) in enumerate(self.groups):
      h = cfg.history_length - 1
      if h > 0:
        r = np.ix_(rows, cols)
        self.hist[:, -1, 0, :][r] = (tgt_act[:, cols] - q[:, cols])[rows]
        self.hist[:, -1, 1, :][r] = qd[:, cols][rows]
        self.pushes[r] = 1
      self.tring[k][rows] = 0  # the delay ring holds the post-reset target
      self.tring[k][rows, -1] = tgt_act[:, cols][rows]
    self.tpush[rows] = 1

  def assert_engine_equal(self, what):
    eng = self.rig.engine
    if self.Hm == 0:
      assert eng.hist is None
      return
    hist = eng.hist.cpu().numpy()[:, :, :, self.gid]
    pushes = eng.hpush.cpu().numpy()[:, self.gid]
    for k, (cols, cfg, lag) in enumerate(self.groups):
      assert np.array_equal(pushes[:, cols], self.pushes[:, cols]), f"{what}: pushes"
      assert np.array_equal(hist[:, :, :, cols].view(np.uint32), self.hist[:, :, :, cols].view(np.uint32)), \
        f"{what}: history frames"
      if lag:
        ring = eng.ring.cpu().numpy()[:, :, self.gid][:, :, cols]
        assert np.array_equal(ring, self.tring[k][:, -ring.shape[1]:]), f"{what}: delayed targets"
        assert np.array_equal(eng.pushes.cpu().numpy()[:, self.gid][:, cols],
                              np.minimum(self.tpush, ring.shape[1])[:, None].repeat(len(cols), 1))


def _k_act(nets, rig, mirror, tgt_act, q, qd, device):
  """k_tanh / k_elu measured on the device over this test's pre-activation range."""
  k = {}
  for i, (cols, cfg, _) in enumerate(mirror.groups):
    layers = nets[cfg.shape][1]
    for name in {l[2] for l in layers} & {"tanh", "elu"}:
      pe, v = mirror.frames(i, tgt_act, q, qd)
      lo, hi = lr.pre_activation_range(layers, lr.inputs(pe, v, cfg.pos_scale, cfg.vel_scale, cfg.input_order))
      k[name] = max(k.get(name, 0.0), lr.measure_k(name, lo, hi, device))
      print(f"k_{name} = {k[name]:.3f} on [{lo:.2f}, {hi:.2f}]")
  return k


def _check_ctrl(nets, rig, mirror, tgt_act, q, qd, k, what, vacuity=False):
  """data.ctrl of the learned actuators against the reference on the mirror's frames; returns
  (clipped, free) counts."""
  ctrl = rig.sim.data.ctrl.cpu().numpy()[:, mirror.gid]
  clipped = free = 0
  for i, (cols, cfg, _) in enumerate(mirror.groups):
    layers = nets[cfg.shape][1]
    pe, v = mirror.frames(i, tgt_act, q, qd)
    ref, bound, clip = lr.ctrl_ref(layers, pe, v, cfg, k)
    lr.check(ctrl[:, cols], ref, bound, f"{what} [{cfg.shape}]")
    clipped, free = clipped + int(clip.sum()), free + int((~clip).sum())
    if vacuity:  # the bound tells a wrong input order and wrong lags from the right ones
      other = "vel_pos" if cfg.input_order == "pos_vel" else "pos_vel"
      wrong = [lr.ctrl_ref(layers, pe, v, cfg, k, order=other)[0]]
      if cfg.history_length > 1:
        wrong.append(lr.ctrl_ref(layers, pe[..., ::-1].copy(), v[..., ::-1].copy(), cfg, k)[0])
      for wr in wrong:
        rows = (np.abs(ctrl[:, cols] - wr) > bound).any(axis=1)
        assert rows.mean() >= 0.5, f"{what}: a wrong reference is within the bound in {1 - rows.mean():.2f} of the rows"
  return clipped, free


def _start(nets, case, device, seed, engine=True, capacity=None, vel_scale=0.5):
  """A rig after a reset of every world at seeded states (primed with the post-reset frame),
  and its mirror."""
  rig = _rig(nets, case, device, engine=engine, capacity=capacity)
  q, qv = _states(rig, seed=seed, vel_scale=vel_scale)
  rig.load(q, qv)
  mirror = Mirror(rig)
  tgt0 = rig.robot.data.joint_pos_target.cpu().numpy()[:, rig.robot._act_joint_local].astype(F32)
  qa, va = mirror.state()
  mirror.prime(np.ones(rig.n, bool), tgt0, qa, va)
  return rig, mirror


def _substep(rig, mirror, tgt, tgt_act):
  """One engine substep with the mirror following; returns the state it started from."""
  q, qd = mirror.state()
  rig.target(tgt)
  rig.env_step(nsub=1)
  mirror.push(tgt_act, q, qd)
  return q, qd


# ------------------------------------------------------------------ 1. one forward
@pytest.mark.parametrize("case", list(CASES))
@guarded
def test_forward_against_the_fp64_reference(case, nets, gpu_device):
  # (joint speeds of a few rad/s, on both sides of the no-load speed; the history is the
  # post-reset frame, the chain test below runs on longer ones)
  rig, mirror = _start(nets, case, gpu_device, seed=31, vel_scale=2.0)
  mirror.assert_engine_equal("after the reset")
  if CASES[case][3]:  # delayed: right after the reset the late target is the reset's own, and
    for sub in range(3):  # every lag would hold the same frame: three substeps, a new target each
      _substep(rig, mirror, *_rand_targets(rig, seed=320 + sub))
    # ... and back to the seeded state: the stiff torque-speed line leaves the joints past its
    # corner after a substep, where the clip alone decides the torque
    q0, qv0 = _states(rig, seed=31, vel_scale=2.0)
    rig.sim.data.qpos[:] = torch.as_tensor(q0, dtype=torch.float32, device=gpu_device)
    rig.sim.data.qvel[:] = torch.as_tensor(qv0, dtype=torch.float32, device=gpu_device)
  tgt, tgt_act = _rand_targets(rig, seed=33)
  q, qd = mirror.state()
  rig.target(tgt)
  rig.scene.write_data_to_sim()
  rig.sim.forward()
  mirror.assert_engine_equal("a forward pushes nothing")
  k = _k_act(nets, rig, mirror, tgt_act, q, qd, gpu_device)
  clipped, free = _check_ctrl(nets, rig, mirror, tgt_act, q, qd, k, f"({case}) engine forward", vacuity=True)
  assert clipped > 0 and free > 0, (clipped, free)
  d = rig.sim.data
  learned = np.concatenate([mirror.gid[c] for c, _, _ in mirror.groups])
  df = (d.actuator_force[:, learned].double() - d.ctrl[:, learned].double()).abs()
  assert torch.equal(d.actuator_force[:, learned], d.ctrl[:, learned]), \
    f"actuator_force != ctrl in {int((df > 0).sum())} of {df.numel()} (NaN {int(df.isnan().sum())}), max {float(df.nan_to_num().max()):.3e}"
  # the torch-mode twin at the same state and history: within its own bound of the same reference
  twin = _rig(nets, case, gpu_device, engine=False)
  st = {f: getattr(rig.sim.data, f).clone() for f in ("qpos", "qvel")}
  rig.sim.clear_explicit_actuators()  # hands the history to the torch buffers ...
  for a_from, a_to in zip(rig.robot.custom_actuators, twin.robot.custom_actuators):
    bf = getattr(a_from, "base_actuator", a_from)
    bt = getattr(a_to, "base_actuator", a_to)
    if hasattr(bf, "_pos_error_history") and bf._pos_error_history.is_initialized:
      for name in ("_pos_error_history", "_vel_history"):
        src, dst = getattr(bf, name), getattr(bt, name)
        dst.append(src.buffer[:, -1])
        dst.buffer.copy_(src.buffer)
        dst.num_pushes.copy_(src.num_pushes)
    if hasattr(a_from, "_delay_buffers"):
      src, dst = a_from._delay_buffers["position"], a_to._delay_buffers["position"]
      dst.append(src._buffer.buffer[:, -1])
      dst._buffer.buffer.copy_(src._buffer.buffer)
      dst._buffer.num_pushes.copy_(src._buffer.num_pushes)
  twin.sim.data.qpos[:] = st["qpos"]
  twin.sim.data.qvel[:] = st["qvel"]
  twin.target(tgt)
  twin.scene.write_data_to_sim()
  twin.sim.forward()
  _check_ctrl(nets, twin, mirror, tgt_act, q, qd, k, f"({case}) torch forward")


# ------------------------------------------------------------------ 2. substep chain against a mirror
@pytest.mark.parametrize("case", list(CASES))
@guarded
def test_substep_chain_follows_the_mirror(case, nets, gpu_device):
  rig, mirror = _start(nets, case, gpu_device, seed=41)
  tgt, tgt_act = _rand_targets(rig, seed=42)
  q, qd = mirror.state()
  for sub in range(8):
    if sub == 4:
      tgt, tgt_act = _rand_targets(rig, seed=43)
    q, qd = mirror.state()
    pre = mirror.copy()
    k = _k_act(nets, rig, pre, tgt_act, q, qd, gpu_device)  # on this substep's own range
    _substep(rig, mirror, tgt, tgt_act)
    mirror.assert_engine_equal(f"({case}) substep {sub}")
    _check_ctrl(nets, rig, pre, tgt_act, q, qd, k, f"({case}) substep {sub}")
  for cols, cfg, _ in mirror.groups:
    assert (mirror.pushes[:, cols] == cfg.history_length - 1).all()


# ------------------------------------------------------------------ 3. one launch = repeated launches
def _hist_state(rig):
  e = rig.engine
  out = {"hpush": e.hpush.clone()} if e.hpush is not None else {}
  if e.hist is not None:
    out["hist"] = e.hist.clone()
  if e.ring is not None:
    out["ring"], out["pushes"] = e.ring.clone(), e.pushes.clone()
  return out


@pytest.mark.parametrize("case,graph,capacity", [("b", False, None), ("c", False, None), ("e", False, None),
                                                 ("f", True, None), ("e", True, None),
                                                 ("e", False, (20, 80))])
@guarded
def test_step4_equals_four_step1(case, graph, capacity, nets, gpu_device):
  """Every DATA_FIELDS field, ctrl and the history, bit for bit; at the small carve the overflow
  re-solve runs phase A twice for the listed worlds (no double push)."""
  a = _rig(nets, case, gpu_device, capacity=capacity)
  b = _rig(nets, case, gpu_device, capacity=capacity)
  q, qv = _states(a, seed=21 if capacity else 51)
  for r in (a, b):
    r.load(q, qv)
  ga = gb = None
  if graph:
    graphs = []
    for r, nsub, reps in ((a, 4, 1), (b, 1, 4)):
      side = torch.cuda.Stream()
      side.wait_stream(torch.cuda.current_stream())
      with torch.cuda.stream(side):
        r.scene.write_data_to_sim()
        r.sim.step(nsub)  # warm the launch path outside capture
      torch.cuda.current_stream().wait_stream(side)
      torch.cuda.synchronize()
      g = torch.cuda.CUDAGraph()
      with torch.cuda.graph(g):
        r.scene.write_data_to_sim()
        for _ in range(reps):
          r.sim.step(nsub)
      graphs.append(g)
      r.load(q, qv)
    ga, gb = graphs
  for step in range(3):
    tgt, _ = _rand_targets(a, seed=60 + step)
    for r in (a, b):
      r.target(tgt)
    if graph:
      ga.replay()
      gb.replay()
    else:
      a.scene.write_data_to_sim()
      a.sim.step(4)
      b.scene.write_data_to_sim()
      for _ in range(4):
        b.sim.step(1)
    torch.cuda.synchronize()
    _assert_equal(a.fields(), b.fields(), f"({case}) env step {step}")
    ha, hb = _hist_state(a), _hist_state(b)
    assert ha.keys() == hb.keys() and "hist" in ha
    for name in ha:
      assert torch.equal(ha[name], hb[name]), (case, step, name)
  assert torch.isfinite(a.sim.data.qpos).all()
  if capacity:
    assert a.sim.stats()["resolved"] > 0 and b.sim.stats()["resolved"] > 0


# ------------------------------------------------------------------ 4. reset
@pytest.mark.parametrize("case", ["b", "e", "f"])
@guarded
def test_masked_reset_in_mid_run(case, nets, gpu_device):
  rig, mirror = _start(nets, case, gpu_device, seed=71)
  tgt, tgt_act = _rand_targets(rig, seed=72)
  for _ in range(3):
    _substep(rig, mirror, tgt, tgt_act)
  before = _hist_state(rig)
  rows = np.zeros(rig.n, bool)
  rows[::3] = True
  mask = torch.as_tensor(rows, device=gpu_device)
  rig.scene.reset_masked(mask)
  q0, qv0 = _states(rig, seed=73)
  rig.sim.data.qpos[mask] = torch.as_tensor(q0, dtype=torch.float32, device=gpu_device)[mask]
  rig.sim.data.qvel[mask] = torch.as_tensor(qv0, dtype=torch.float32, device=gpu_device)[mask]
  rig.scene.write_data_to_sim(mask=mask)
  rig.sim.forward()
  after = _hist_state(rig)
  for name in before:
    assert torch.equal(before[name][~mask], after[name][~mask]), f"{name} of the other worlds"
  q, qd = mirror.state()
  pt = rig.robot.data.joint_pos_target.cpu().numpy()[:, rig.robot._act_joint_local].astype(F32)
  mirror.prime(rows, pt, q, qd)
  mirror.assert_engine_equal("after the masked reset")
  gid = mirror.gid
  for cols, cfg, _ in mirror.groups:
    assert (rig.engine.hpush.cpu().numpy()[:, gid][rows][:, cols] == 1).all()
  tgt2 = np.where(rows[:, None], rig.robot.data.joint_pos_target.cpu().numpy(), tgt).astype(F32)
  tgt2_act = tgt2[:, rig.robot._act_joint_local]
  pre = mirror.copy()
  k = _k_act(nets, rig, pre, tgt2_act, q, qd, gpu_device)
  _substep(rig, mirror, tgt2, tgt2_act)
  mirror.assert_engine_equal("the substep after the reset")
  _check_ctrl(nets, rig, pre, tgt2_act, q, qd, k, f"({case}) after the reset")


# ------------------------------------------------------------------ 5. binding
@guarded
def test_binding_hands_the_history_over_and_back(nets, gpu_device):
  rig, mirror = _start(nets, "b", gpu_device, seed=81)
  tgt, tgt_act = _rand_targets(rig, seed=82)
  for _ in range(3):
    _substep(rig, mirror, tgt, tgt_act)
  rig.sim.clear_explicit_actuators()
  rig.engine = None
  assert rig.sim.explicit_actuators is None and rig.robot._engine_actuators is None
  k = {}
  q, qd = mirror.state()
  rig.env_step(nsub=1)  # torch path: write_data_to_sim + step(1)
  _check_ctrl(nets, rig, mirror, tgt_act, q, qd, k, "torch path after the hand-back")
  mirror.push(tgt_act, q, qd)
  rig.engine = rig.sim.set_explicit_actuators(rig.scene.entities.values())
  mirror.assert_engine_equal("rebound")
  q, qd = mirror.state()
  pre = mirror.copy()
  _substep(rig, mirror, tgt, tgt_act)
  mirror.assert_engine_equal("a substep after rebinding")
  _check_ctrl(nets, rig, pre, tgt_act, q, qd, k, "engine after rebinding")


@guarded
def test_unextractable_module_and_wrong_kind_are_refused(nets, gpu_device):
  from mjlab_amd._lib import lib
  from mjlab_amd.actuator import ActuatorNetDesc
  bad = Rig(GO1, _learned(nets, "layernorm"), 8, gpu_device)
  with pytest.raises(ValueError, match="LayerNorm"):
    bad.sim.set_explicit_actuators(bad.scene.entities.values())
  assert bad.sim.explicit_actuators is None
  # more networks than the engine holds: refused before any actuator's state is touched
  many = Rig(G1, _learned(nets, "b", tscale=lambda lim: 3.0 * lim), 8, gpu_device)  # five scales
  before = [(a.stiffness.data_ptr(), a._engine) for a in many.robot.custom_actuators]
  with pytest.raises(ValueError, match="more than 4 different actuator networks"):
    many.sim.set_explicit_actuators(many.scene.entities.values())
  assert many.sim.explicit_actuators is None and many.robot._engine_actuators is None
  assert before == [(a.stiffness.data_ptr(), a._engine) for a in many.robot.custom_actuators]
  assert all(e is None for _, e in before)
  # net[u] on an ideal-PD actuator (kind 2)
  r = _rig(nets, "e", gpu_device)
  L = lib()
  d = ActuatorNetDesc.from_buffer_copy(r.engine.net_desc)
  nu = d.nu
  table = (ctypes.c_uint8 * nu)(*[0] * nu)
  d.net = ctypes.cast(table, ctypes.c_void_p)
  assert L.mjx_sim_set_actuator_nets(r.sim._sim, ctypes.addressof(d), None) != 0
  why = L.mjx_last_error().decode()
  assert "mjx_sim_set_actuator_nets" in why and "kind is not 3" in why
  r.sim.step(1)  # the earlier binding stands
  assert torch.isfinite(r.sim.data.qpos).all()


# ------------------------------------------------------------------ 6. fused env
@pytest.mark.parametrize("task", [G1, GO1])
@guarded
def test_fused_env_runs_learned_actuators_in_engine_mode(task, nets, gpu_device):
  """Every group learned (shape b): the fused step is built and engine mode bound; ten captured
  steps, a third of the envs timing out at step 3, against the unfused sync-free env in engine
  mode.  Physics state and the network history bit for bit; observations and rewards as
  tests/test_gpu_actuators.py compares them."""
  make = lambda i, g: _learned(nets, "b_small")(g)
  et = _env(task, make, gpu_device, fused=False, capture=False)
  ef = _env(task, make, gpu_device, fused=True, capture=True)
  assert ef._fused is not None, getattr(ef, "_fused_unsupported", "")
  eng = ef.sim.explicit_actuators
  assert eng is not None and ef._fused._engine_act is eng and eng.hist is not None
  assert et._fused is None
  engt = et.sim.set_explicit_actuators(et.scene.entities.values())
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
      print(f"{task} step {step}: {k} max |diff| {d:.3e}")
      assert torch.equal(x, y), (step, k, d)
    assert torch.equal(engt.hist, eng.hist) and torch.equal(engt.hpush, eng.hpush), step
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
      assert (eng.hpush[::3] == 1).all() and (eng.hpush[1::3] == 2).all()
  # (without a position loop the robots sag, and more envs terminate than the timed-out third)
  assert ef._graph is not None and was_reset.any()
  assert (ef.sim.data.ctrl.abs() > 0).any()


@guarded
def test_fused_env_reports_an_unextractable_network(nets, gpu_device):
  e = _env(GO1, lambda i, g: _learned(nets, "layernorm")(g), gpu_device, fused=True, capture=False)
  assert e._fused is None and "LayerNorm" in e._fused_unsupported
  assert e.sim.explicit_actuators is None
  nact = e.action_manager.total_action_dim
  for _ in range(2):
    e.step(torch.zeros(ENV_N, nact, device=gpu_device))
  assert torch.isfinite(e.sim.data.qpos).all()
