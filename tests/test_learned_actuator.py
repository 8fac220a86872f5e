"""The learned (MLP) actuator on the CPU: the torch form against the fp64 reference of
tests/learned_ref.py (bound and derivation there), the cfg, the extraction of a TorchScript
module into a plain MLP, and the descriptor checks of mjx_sim_set_actuator_nets.  The engine
form is checked on the GPU (tests/test_gpu_learned_actuator.py)."""

import ctypes
import os
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from torch import nn

import learned_ref as lr
from mjlab_amd.actuator import (ActuatorCmd, DelayedActuatorCfg, LearnedMlpActuator,
                                LearnedMlpActuatorCfg, engine_unsupported, extract_mlp)

N, NJ = 6, 3
ACT = {"relu": nn.ReLU, "softsign": nn.Softsign, "tanh": nn.Tanh, "elu": nn.ELU}


def _cfg(path, H=3, order="pos_vel", **kw):
  kw.setdefault("effort_limit", 4.0)
  kw.setdefault("saturation_effort", 6.0)
  kw.setdefault("velocity_limit", 20.0)
  with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    return LearnedMlpActuatorCfg(joint_names_expr=("joint.*",), network_file=path, pos_scale=1.7,
                                 vel_scale=0.11, torque_scale=9.0, input_order=order,
                                 history_length=H, **kw)


def _build(cfg, n=N, nj=NJ):
  joints = [f"joint{i}" for i in range(nj)]
  act = cfg.build(None, list(range(nj)), joints)
  act._ctrl_ids_list = list(range(nj))
  act.initialize(None, None, SimpleNamespace(qpos=torch.zeros(n, 1)), "cpu")
  return act


def _states(seed, steps, n=N, nj=NJ):
  g = torch.Generator().manual_seed(seed)
  r = lambda s: (torch.rand(steps, n, nj, generator=g) * 2 - 1) * s
  return r(1.0), r(0.8), r(12.0)  # targets, positions, velocities


def _cmd(pt, q, qd):
  z = torch.zeros_like(pt)
  return ActuatorCmd(position_target=pt, velocity_target=z, effort_target=z, joint_pos=q, joint_vel=qd)


def _k(layers, name):
  if name not in ("tanh", "elu"):
    return {}
  return {name: lr.measure_k(name, -8.0, 8.0)}


@pytest.mark.parametrize("H,order,act", [(1, "pos_vel", "relu"), (3, "pos_vel", "softsign"),
                                         (3, "vel_pos", "softsign"), (8, "vel_pos", "tanh"),
                                         (3, "pos_vel", "elu")])
def test_torch_form_against_the_fp64_reference(tmp_path, H, order, act):
  """Five consecutive compute calls: backfill on the first, the scales, both input orders, the
  DC clip binding for some rows and not for others."""
  seq = lr.make_net([2 * H, 16, 5, 1] if H > 1 else [2, 1], ACT[act], seed=3 + H)
  cfg = _cfg(lr.save_net(seq, tmp_path / "net.pt"), H, order)
  a = _build(cfg)
  layers, k = lr.layers_of(seq), _k(None, act)
  mirror = lr.History(N, NJ, H)
  pt, q, qd = _states(11, 5)
  clipped = free = 0
  for s in range(5):
    out = a.compute(_cmd(pt[s], q[s], qd[s])).numpy()
    mirror.append((pt[s] - q[s]).numpy(), qd[s].numpy())
    if s == 0:  # backfill: every lag holds the first frame
      assert (mirror.pe == mirror.pe[..., :1]).all()
    ref, bound, clip = lr.ctrl_ref(layers, mirror.pe, mirror.qd, cfg, k)
    lr.check(out, ref, bound, f"H={H} {order} {act} step {s}")
    clipped += int(clip.sum())
    free += int((~clip).sum())
    if H > 1 and s > 0:  # the bound is not vacuous: the other input order is another answer
      other = "vel_pos" if order == "pos_vel" else "pos_vel"
      wrong, _, _ = lr.ctrl_ref(layers, mirror.pe, mirror.qd, cfg, k, order=other)
      assert lr.differs(out, wrong, bound) > 0.5
  assert clipped > 0 and free > 0, (clipped, free)


def test_reset_of_a_subset_leaves_the_other_rows_bit_for_bit(tmp_path):
  seq = lr.make_net([6, 8, 1], nn.Softsign, seed=5)
  cfg = _cfg(lr.save_net(seq, tmp_path / "net.pt"))
  a, b = _build(cfg), _build(cfg)
  layers = lr.layers_of(seq)
  pt, q, qd = _states(12, 6)
  mirror = lr.History(N, NJ, 3)
  for s in range(3):
    a.compute(_cmd(pt[s], q[s], qd[s]))
    b.compute(_cmd(pt[s], q[s], qd[s]))
    mirror.append((pt[s] - q[s]).numpy(), qd[s].numpy())
  rows = torch.tensor([1, 4])
  a.reset(rows)
  mirror.reset(rows.numpy())
  assert a._pos_error_history.num_pushes.tolist() == [3, 0, 3, 3, 0, 3]
  keep = np.array([0, 2, 3, 5])
  for s in range(3, 6):
    oa = a.compute(_cmd(pt[s], q[s], qd[s])).numpy()
    ob = b.compute(_cmd(pt[s], q[s], qd[s])).numpy()
    mirror.append((pt[s] - q[s]).numpy(), qd[s].numpy())
    assert np.array_equal(oa[keep], ob[keep])  # untouched rows: the same bits as without the reset
    ref, bound, _ = lr.ctrl_ref(layers, mirror.pe, mirror.qd, cfg, {})
    lr.check(oa, ref, bound, f"after reset, step {s}")
  # reset_masked is the same reset
  a.reset_masked(torch.tensor([True, False, False, False, False, False]))
  assert a._vel_history.num_pushes.tolist() == [0, 3, 6, 6, 3, 6]


def test_masked_compute_keeps_history_and_output_of_the_other_rows(tmp_path):
  seq = lr.make_net([6, 8, 1], nn.ReLU, seed=6)
  cfg = _cfg(lr.save_net(seq, tmp_path / "net.pt"))
  a = _build(cfg)
  layers = lr.layers_of(seq)
  pt, q, qd = _states(13, 5)
  mirror = lr.History(N, NJ, 3)
  for s in range(3):
    last = a.compute(_cmd(pt[s], q[s], qd[s])).clone()
    mirror.append((pt[s] - q[s]).numpy(), qd[s].numpy())
  before = [t.clone() for t in (a._pos_error_history.buffer, a._vel_history.buffer,
                                a._pos_error_history.num_pushes)]
  mask = torch.tensor([True, False, True, False, False, True])
  out = a.compute(_cmd(pt[3], q[3], qd[3]), mask=mask)
  mirror.append((pt[3] - q[3]).numpy(), qd[3].numpy(), rows=mask.numpy())
  after = (a._pos_error_history.buffer, a._vel_history.buffer, a._pos_error_history.num_pushes)
  for x, y in zip(before, after):
    assert torch.equal(x[~mask], y[~mask])
  assert a._pos_error_history.num_pushes.tolist() == [4, 3, 4, 3, 3, 4]
  assert torch.equal(out[~mask], last[~mask])
  ref, bound, _ = lr.ctrl_ref(layers, mirror.pe, mirror.qd, cfg, {})
  lr.check(out[mask].numpy(), ref[mask.numpy()], bound[mask.numpy()], "masked rows")
  out = a.compute(_cmd(pt[4], q[4], qd[4])).numpy()  # then every row goes on from its own history
  mirror.append((pt[4] - q[4]).numpy(), qd[4].numpy())
  ref, bound, _ = lr.ctrl_ref(layers, mirror.pe, mirror.qd, cfg, {})
  lr.check(out, ref, bound, "after the masked call")


def test_learned_actuator_behind_a_fixed_delay(tmp_path):
  seq = lr.make_net([6, 8, 1], nn.Softsign, seed=7)
  cfg = _cfg(lr.save_net(seq, tmp_path / "net.pt"))
  a = _build(DelayedActuatorCfg(base_cfg=cfg, delay_min_lag=2, delay_max_lag=2))
  assert isinstance(a.base_actuator, LearnedMlpActuator)
  layers = lr.layers_of(seq)
  pt, q, qd = _states(14, 5)
  mirror = lr.History(N, NJ, 3)
  for s in range(5):
    out = a.compute(_cmd(pt[s], q[s], qd[s])).numpy()
    late = pt[max(s - 2, 0)]  # lag 2, clamped to the frames held
    mirror.append((late - q[s]).numpy(), qd[s].numpy())
    ref, bound, _ = lr.ctrl_ref(layers, mirror.pe, mirror.qd, cfg, {})
    lr.check(out, ref, bound, f"delayed, step {s}")
  # a masked call reaches the base actuator's history as well
  mask = torch.tensor([True] + [False] * (N - 1))
  a.compute(_cmd(pt[0], q[0], qd[0]), mask=mask)
  assert a.base_actuator._pos_error_history.num_pushes.tolist() == [6] + [5] * (N - 1)


def test_cfg_defaults_and_the_compiled_group(tmp_path):
  with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    cfg = LearnedMlpActuatorCfg(joint_names_expr=("j.*",), network_file="x.pt", pos_scale=1.0,
                                vel_scale=1.0, torque_scale=1.0, effort_limit=7.0,
                                saturation_effort=9.0, velocity_limit=30.0, armature=0.01)
  # the reference's defaults (learned_actuator.py:46-62)
  assert (cfg.input_order, cfg.history_length, cfg.stiffness, cfg.damping) == ("pos_vel", 3, 0.0, 0.0)
  g = cfg.compile_group()
  assert type(g).__name__ == "MotorActuatorGroup" and g.effort_limit == 7.0 and g.armature == 0.01
  assert DelayedActuatorCfg(base_cfg=cfg, delay_max_lag=1).compile_group().effort_limit == 7.0
  with pytest.raises(ValueError, match="Invalid input order"):
    _build(_cfg(lr.save_net(lr.make_net([6, 1], nn.ReLU, 1), tmp_path / "n.pt"), order="pos"))
  from mjlab_amd import entity
  assert entity.LearnedMlpActuatorCfg is LearnedMlpActuatorCfg


# ------------------------------------------------------------------ extraction
@pytest.mark.parametrize("widths,act,H", [([2, 1], "relu", 1), ([6, 32, 32, 32, 1], "softsign", 3),
                                          ([16, 5, 1], "tanh", 8), ([6, 8, 1], "elu", 3),
                                          ([4, 7, 1], "relu", 2)])
@pytest.mark.parametrize("how", ["script", "trace"])
def test_extraction_round_trips(tmp_path, widths, act, H, how):
  seq = lr.make_net(widths, ACT[act], seed=21)
  mod = torch.jit.script(seq) if how == "script" else torch.jit.trace(seq, torch.zeros(3, widths[0]))
  mod.save(str(tmp_path / "m.pt"))
  spec, why = extract_mlp(torch.jit.load(str(tmp_path / "m.pt")), H)
  assert why is None and spec.widths == widths
  for (W, b, name), w2, b2, code in zip(lr.layers_of(seq), spec.weights, spec.biases, spec.activations):
    assert np.array_equal(W, w2.double().numpy()) and np.array_equal(b, b2.double().numpy())
    assert ["none", "relu", "softsign", "tanh", "elu"][code] == name


class _Scaled(nn.Module):  # children that look like an MLP, a forward that is not one
  def __init__(self):
    super().__init__()
    self.a = nn.Linear(6, 4)
    self.b = nn.Linear(4, 1)

  def forward(self, x):
    return self.b(self.a(x)) * 2.0


@pytest.mark.parametrize("make,H,word", [
    (lambda: nn.Sequential(nn.Linear(6, 8), nn.LayerNorm(8), nn.Linear(8, 1)), 3, "LayerNorm"),
    (lambda: lr.make_net([6, 33, 1], nn.ReLU, 1), 3, "width 33"),
    (lambda: lr.make_net([6, 4, 4, 4, 4, 1], nn.ReLU, 1), 3, "5 linear layers"),
    (lambda: lr.make_net([18, 4, 1], nn.ReLU, 1), 9, "history_length 9"),
    (lambda: nn.Sequential(nn.Linear(6, 4, bias=False), nn.ReLU(), nn.Linear(4, 1)), 3, "without a bias"),
    (lambda: nn.Sequential(nn.Linear(6, 1), nn.Tanh()), 3, "after the last layer"),
    (lambda: nn.Sequential(nn.Linear(6, 4), nn.ELU(alpha=0.5), nn.Linear(4, 1)), 3, "alpha"),
    (lambda: lr.make_net([8, 4, 1], nn.ReLU, 1), 3, "input width 8"),
    (lambda: lr.make_net([6, 4, 2], nn.ReLU, 1), 3, "output width 2"),
    (_Scaled, 3, "not the plain MLP"),
])
def test_extraction_gives_a_reason(tmp_path, make, H, word):
  torch.jit.script(make()).save(str(tmp_path / "m.pt"))
  spec, why = extract_mlp(torch.jit.load(str(tmp_path / "m.pt")), H)
  assert spec is None and word in why, why


def test_engine_unsupported_reports_the_reason(tmp_path):
  ok = _build(_cfg(lr.save_net(lr.make_net([6, 8, 1], nn.Tanh, 2), tmp_path / "a.pt")))
  assert engine_unsupported(ok) is None
  bad = nn.Sequential(nn.Linear(6, 8), nn.LayerNorm(8), nn.Linear(8, 1))
  act = _build(_cfg(lr.save_net(bad, tmp_path / "b.pt")))
  assert "LayerNorm" in engine_unsupported(act)
  wrapped = _build(DelayedActuatorCfg(base_cfg=_cfg(str(tmp_path / "b.pt")), delay_max_lag=1))
  assert "LayerNorm" in engine_unsupported(wrapped)
  out = act.compute(_cmd(*[t[0] for t in _states(1, 1)]))  # the torch path runs any module
  assert out.shape == (N, NJ) and torch.isfinite(out).all()


# ------------------------------------------------------------------ C ABI
def test_bad_net_descriptors_return_an_error_code():
  """mjx_sim_set_actuator_nets checks the descriptor's own consistency before it looks at the
  sim: every refusal below is reached without a GPU, and a consistent descriptor then fails on
  the null sim."""
  lib_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mjlab-1_amd",
                          "mjlab_amd", "libmjx355.so")
  if not os.path.exists(lib_path):
    pytest.skip("libmjx355.so not built (run __graft_entry__.build())")
  from mjlab_amd.actuator import ActuatorNetDesc
  L = ctypes.CDLL(lib_path)
  L.mjx_last_error.restype = ctypes.c_char_p
  L.mjx_actuator_net_desc_size.restype = ctypes.c_size_t
  assert L.mjx_actuator_net_desc_size() == ctypes.sizeof(ActuatorNetDesc)
  L.mjx_sim_set_actuator_nets.argtypes = [ctypes.c_void_p] * 3
  nu = 3
  store = (ctypes.c_float * 4096)()  # weights are read only after the sim is checked
  somewhere = ctypes.cast(store, ctypes.c_void_p).value
  u8 = lambda v: ctypes.cast((ctypes.c_uint8 * nu)(*v), ctypes.c_void_p)
  keep = []

  def call(net=(0, 255, 1), nets=None, **edit):
    d = ActuatorNetDesc()
    d.nworld, d.nu, d.nnet, d.hist_len = 2, nu, 2, 2
    for k, (widths, acts, H) in enumerate((((6, 8, 1), (1, 0), 3), ((2, 1), (0,), 1))):
      e = d.nets[k]
      e.nlayer, e.history, e.input_order = len(widths) - 1, H, k
      e.pos_scale = e.vel_scale = e.torque_scale = 1.0
      for l, w in enumerate(widths):
        e.width[l] = w
      for l, a in enumerate(acts):
        e.activation[l], e.weight[l], e.bias[l] = a, somewhere, somewhere
    if net is not None:
      keep.append(u8(net))
      d.net = keep[-1]
    d.history = d.staging = d.pushes = somewhere
    for k, v in edit.items():
      setattr(d, k, v)
    if nets:
      nets(d.nets)
    rc = L.mjx_sim_set_actuator_nets(None, ctypes.byref(d), None)
    return rc, L.mjx_last_error().decode()

  def net_edit(k, **kw):
    def f(nets):
      for name, v in kw.items():
        if isinstance(v, tuple):
          getattr(nets[k], name)[v[0]] = v[1]
        else:
          setattr(nets[k], name, v)
    return f

  cases = [(dict(nworld=0), "nworld"), (dict(nu=0), "nu"), (dict(nu=65), "nu"),
           (dict(nnet=0), "nnet"), (dict(nnet=5), "nnet"), (dict(hist_len=1), "hist_len"),
           (dict(net=None), "null net table"), (dict(net=(0, 2, 1)), "net[u] out of range"),
           (dict(net=(255, 255, 255)), "no actuator has a network"),
           (dict(history=None), "null history"), (dict(staging=None), "null history"),
           (dict(pushes=None), "null history"),
           (dict(nets=net_edit(0, nlayer=0)), "nlayer"), (dict(nets=net_edit(0, nlayer=5)), "nlayer"),
           (dict(nets=net_edit(1, history=0)), "history"), (dict(nets=net_edit(0, history=9)), "history"),
           (dict(nets=net_edit(0, input_order=2)), "input_order"),
           (dict(nets=net_edit(0, width=(1, 33))), "width"), (dict(nets=net_edit(0, width=(1, 0))), "width"),
           (dict(nets=net_edit(0, width=(0, 8))), "2 * history"),
           (dict(nets=net_edit(0, width=(2, 2))), "output width"),
           (dict(nets=net_edit(0, activation=(0, 5))), "activation must be"),
           (dict(nets=net_edit(0, activation=(1, 3))), "after the last layer"),
           (dict(nets=net_edit(0, weight=(1, None))), "null weight"),
           (dict(nets=net_edit(1, bias=(0, None))), "null weight")]
  for edit, why in cases:
    rc, msg = call(**edit)
    assert rc != 0 and "mjx_sim_set_actuator_nets" in msg and why in msg, (edit, msg)
  rc, msg = call()  # consistent: only the sim is missing
  assert rc != 0 and "mjx_sim_set_actuator_nets" in msg and "null sim" in msg
  rc, msg = call(net=(1, 1, 255), nnet=2)  # (history buffers unused by net 1 alone still given)
  assert rc != 0 and "null sim" in msg
  assert L.mjx_sim_set_actuator_nets(None, None, None) != 0 and b"null sim" in L.mjx_last_error()
